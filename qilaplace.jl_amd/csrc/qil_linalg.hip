// Device dense linear algebra used by compress!/canonicalize!/signal_mps/rsvd:
//   GEMM (f64 / c64, N/T/H operands), one-sided Jacobi SVD, Gram-Schmidt QR with positive
//   diagonal, counter-based Gaussian fill, and the ITensors truncation rule.
//
// The reference delegates all of this to ITensors.jl -> LAPACK/BLAS (not in its tree):
//   svd   src/mps.jl:929,946; src/signals/SignalConverters.jl:84,266; src/linalg/rsvd.jl:103
//   qr    src/linalg/rsvd.jl:83,90,94 (positive=true)
//   `*`   every contraction on the path
// Only gauge-invariant results are comparable with the reference.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include <utility>

#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

// ------------------------------------------------------------------ GEMM on the f64 matrix cores
// C (m x n) = opA(A) * opB(B), f64 or c64, through v_mfma_f64_16x16x4_f64 (64-cycle issue per SIMD).
//   * BM x BN output tile per 256-thread workgroup, 4 waves in a (BM/WM) x (BN/WN) arrangement, each
//     wave WM/16 x WN/16 MFMA tiles (up to 4 x 4 = 64 accumulator doubles per lane);
//   * K tiles of 16; PIPE = true: software pipelined -- the next tile's global loads are issued into
//     registers right after the barrier and land while the current tile's MFMAs run, LDS double buffered,
//     ONE barrier per K tile (f64: fewer registers, 2 waves/SIMD still fit); PIPE = false: single buffer,
//     smaller footprint => 3 waves/SIMD, which the complex kernel (3 accumulator sets) needs to keep the
//     matrix pipe fed.  Built with -amdgpu-mfma-vgpr-form: with AGPR accumulators this MFMA issues at ~0.6 of
//     its rate on gfx950 (46 vs 77.6 TFLOP/s for a pure MFMA stream, tools/micro/mfma_f64_variants.hip);
//   * LDS holds split re/im planes, rows padded by 2 doubles (keeps both the k-major staging writes and
//     the fragment reads at <= 2-way bank conflicts);
//   * the MFMA is issued as (B^T tile) x (A^T tile) = (AB)^T tile: the D fragment then has the C ROW
//     index on lane&15, so every 16 lanes store 128 B (f64) / 256 B (c64) contiguous in column-major C;
//   * complex product = 3 real MFMAs (Gauss, r05) into 3 accumulators (rr = k1, ii = k3, ri = k2): C = (rr - ii) + i (rr + ri);
//   * operands are addressed through (row stride, k stride, conj) so N/T/H/conj need no extra kernels;
//     the global->register mapping follows whichever index is contiguous (coalesced either way);
//   * gridDim.z > 1 = split-K into a workspace + fixed-order reduction (deterministic).
constexpr int GK = 16;
#ifndef QIL_GEMM_GAUSS
#define QIL_GEMM_GAUSS 1          // complex products by three real multiplications (0: four; A/B builds)
#endif
#ifndef QIL_GEMM_PAD
#define QIL_GEMM_PAD 2
#endif
constexpr int GPAD = QIL_GEMM_PAD;   // LDS row padding in doubles
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void put_plane(double* S0, double* S1, int off, double v) {
    S0[off] = v;
    (void)S1;
}
__device__ __forceinline__ void put_plane(double* S0, double* S1, int off, c64 v) {
    S0[off] = v.re;
    S1[off] = v.im;
}
__device__ __forceinline__ double maybe_conj(double v, int) { return v; }
__device__ __forceinline__ c64 maybe_conj(c64 v, int cj) { return cj ? c64{v.re, -v.im} : v; }

// ARC / BKC: op(A)'s row index / op(B)'s k index is the contiguous one in memory (compile time, so that the staging
// pattern -- which element of the tile a thread loads and where it lands in LDS -- folds into constants).
template <class T, int BM, int BN, int WM, int WN, bool PIPE, bool ARC, bool BKC, int GKT = GK, int DEEP = 0>
__device__ __forceinline__ void gemm_mfma_body(const uint3 blockIdx, const uint3 gridDim, long long m, long long n, long long k_total,
                                                 const T* __restrict__ A, long long a_rs, long long a_ks, int conjA,
                                                 const T* __restrict__ B, long long b_ks, long long b_cs, int conjB,
                                                 T* __restrict__ C, long long ldc, long long kchunk,
                                                 long long cstride, int tiles_m, int tiles_n, int col_fastest,
                                                 long long a_bs, long long b_bs, long long c_bs,
                                                 const int* __restrict__ cmap, int cmap_blk,
                                                 const uint8_t* __restrict__ b_sel, long long b_sel_step,
                                                 long long b_sel_stride, int subtract) {
    constexpr bool CX = sizeof(T) == 16;
    constexpr int NP = CX ? 2 : 1;
    constexpr int LA = BM + GPAD, LB = BN + GPAD;   // +2 doubles: <= 2-way LDS conflicts for both the k-major
                                              // staging writes and the fragment reads
    constexpr int NBUF = PIPE ? 2 : 1;
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int EA = BM * GKT / 256, EB = BN * GKT / 256;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per workgroup");
    extern __shared__ __attribute__((aligned(16))) char gemm_smem[];
    double* As = reinterpret_cast<double*>(gemm_smem);            // [NBUF][NP][GKT][LA]
    double* Bs = As + NBUF * NP * GKT * LA;                         // [NBUF][NP][GKT][LB]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = (wave % (BM / WM)) * WM, wc = (wave / (BM / WM)) * WN;
    const int l15 = lane & 15, l4 = lane >> 4;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so workgroup b
    // runs on XCD b % 8.  Give every XCD one CONTIGUOUS eighth of the tile sequence instead of every eighth tile:
    // neighbouring tiles share an operand panel, and now they also share an L2.  The host decides (gemm_plan: at least 64
    // tiles and a multiple of 8 -- an exact split keeps the map a bijection without a table) and says so in bit 1 of col_fastest.
    int tile = blockIdx.x;
    if (col_fastest & 2) tile = (tile % 8) * (tiles_m * tiles_n / 8) + tile / 8;
    int tm, tn;
    if (col_fastest & 1) {
        tn = tile % tiles_n;
        tm = tile / tiles_n;
    } else {
        tm = tile % tiles_m;
        tn = tile / tiles_m;
    }
    const long long row0 = (long long)tm * BM, col0 = (long long)tn * BN;
    const long long kbeg = (long long)blockIdx.z * kchunk;
    const long long kend = min(k_total, kbeg + kchunk);
    // batch = blockIdx.y: strided operands; with `cmap` the output COLUMN BLOCKS of batch y are scattered
    // (block g of width cmap_blk goes to column block cmap[y * n / cmap_blk + g] of the un-strided C)
    A += (long long)blockIdx.y * a_bs;
    B += (long long)blockIdx.y * b_bs;
    // per-batch operand selection: batch y reads B shifted by b_sel[y * step] * stride elements (the lazy
    // coefficient chain picks the output-bit slice of each query this way)
    if (b_sel) B += (long long)b_sel[(long long)blockIdx.y * b_sel_step] * b_sel_stride;
    C += (long long)blockIdx.z * cstride + (long long)blockIdx.y * c_bs;
    if (cmap) cmap += (long long)blockIdx.y * (n / cmap_blk);

    d4 rr[TM][TN], ii[CX ? TM : 1][CX ? TN : 1], ri[CX ? TM : 1][CX ? TN : 1];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            rr[a][b] = d4{0, 0, 0, 0};
            if (CX) {
                ii[a][b] = d4{0, 0, 0, 0};
                ri[a][b] = d4{0, 0, 0, 0};
            }
        }
    // global -> register mapping: fastest along the contiguous index of each operand.  Everything that does
    // not change from K tile to K tile is computed ONCE per thread: a pointer per staged element (advanced by one
    // tile per iteration), its row/column validity, its k offset and its LDS slot.  Inside the loop a load is a
    // compare, two selects and the load itself -- the per-element 64-bit index products used to cost ~20 VALU
    // instructions per element per tile and kept the wave off the matrix pipe.
    constexpr bool a_rows_contig = ARC, b_k_contig = BKC;
    T ra[EA], rb[EB];
    const T* pa[EA];
    const T* pb[EB];
    int ka[EA], kb[EB], sa[EA], sb[EB];
#pragma unroll
    for (int e = 0; e < EA; ++e) {
        const int idx = tid + 256 * e;
        const int i = a_rows_contig ? idx % BM : idx / GKT;
        const int kk = a_rows_contig ? idx / BM : idx % GKT;
        const long long gr = row0 + i;
        ka[e] = kk;
        sa[e] = kk * LA + i;
        pa[e] = A + min(gr, m - 1) * a_rs + (kbeg + kk) * a_ks;
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
        const int idx = tid + 256 * e;
        const int kk = b_k_contig ? idx % GKT : idx / BN;
        const int j = b_k_contig ? idx / GKT : idx % BN;
        const long long gc = col0 + j;
        kb[e] = kk;
        sb[e] = kk * LB + j;
        pb[e] = B + (kbeg + kk) * b_ks + min(gc, n - 1) * b_cs;
    }
    const long long a_step = (long long)GKT * a_ks, b_step = (long long)GKT * b_ks;
    // Edges.  Rows / columns beyond the matrix are CLAMPED to the last valid one when the pointers are set up: such
    // lanes load real data that only ever reaches C entries the epilogue does not store, so the M / N edges need no
    // predicate at all.  Only the K edge matters (a partial last tile would add garbage to valid entries): full
    // tiles -- all but possibly the last -- run plain loads and plain stores to LDS, the last one selects a valid
    // address per lane and zeroes the k-invalid elements when the tile is staged.  Nothing touches a loaded value
    // before store_tile, so the loads stay in flight across the MFMAs of the current tile.
    auto load_tile_into = [&](T(&ra)[EA], T(&rb)[EB], long long k0) {
        if (k0 + GKT <= kend) {
#pragma unroll
            for (int e = 0; e < EA; ++e) {
                ra[e] = *pa[e];
                pa[e] += a_step;
            }
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                rb[e] = *pb[e];
                pb[e] += b_step;
            }
        } else {
#pragma unroll
            for (int e = 0; e < EA; ++e) ra[e] = *((k0 + ka[e] < kend) ? pa[e] : A);
#pragma unroll
            for (int e = 0; e < EB; ++e) rb[e] = *((k0 + kb[e] < kend) ? pb[e] : B);
        }
    };
    auto load_tile = [&](long long k0) { load_tile_into(ra, rb, k0); };
    auto store_tile_from = [&](const T(&ra)[EA], const T(&rb)[EB], int buf, long long k0) {     // k0 = first k of the tile held in ra / rb
        double* a0 = As + (buf * NP) * GKT * LA;
        double* b0 = Bs + (buf * NP) * GKT * LB;
        if (k0 + GKT <= kend) {
#pragma unroll
            for (int e = 0; e < EA; ++e) put_plane(a0, a0 + GKT * LA, sa[e], maybe_conj(ra[e], conjA));
#pragma unroll
            for (int e = 0; e < EB; ++e) put_plane(b0, b0 + GKT * LB, sb[e], maybe_conj(rb[e], conjB));
        } else {
#pragma unroll
            for (int e = 0; e < EA; ++e)
                put_plane(a0, a0 + GKT * LA, sa[e], (k0 + ka[e] < kend) ? maybe_conj(ra[e], conjA) : T{});
#pragma unroll
            for (int e = 0; e < EB; ++e)
                put_plane(b0, b0 + GKT * LB, sb[e], (k0 + kb[e] < kend) ? maybe_conj(rb[e], conjB) : T{});
        }
    };
    auto store_tile = [&](int buf, long long k0) { store_tile_from(ra, rb, buf, k0); };
    auto mfma_tile = [&](int buf) {
        const double* a0 = As + (buf * NP) * GKT * LA;
        const double* b0 = Bs + (buf * NP) * GKT * LB;
#pragma unroll
        for (int kk = 0; kk < GKT; kk += 4) {
            double are[TM], aim[TM], bre[TN], bim[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                are[t] = a0[(kk + l4) * LA + wr + 16 * t + l15];
                if (CX) aim[t] = a0[GKT * LA + (kk + l4) * LA + wr + 16 * t + l15];
            }
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                bre[t] = b0[(kk + l4) * LB + wc + 16 * t + l15];
                if (CX) bim[t] = b0[GKT * LB + (kk + l4) * LB + wc + 16 * t + l15];
            }
            if constexpr (CX && QIL_GEMM_GAUSS) {
                // complex product by Gauss's three multiplications (r05): with k1 = br (ar + ai), k2 = ar (bi - br),
                // k3 = ai (br + bi):  re = k1 - k3,  im = k1 + k2.  Three MFMAs per complex multiply-add instead of four -- the
                // matrix pipe is what a complex product is bound by (64 cycles per v_mfma_f64_16x16x4) --, the three operand sums
                // are VALU adds on the fragments just read (TM + 2 TN per K step of 3 TM TN MFMAs).  Normwise as accurate as the
                // four-multiplication form (error ~ u |a| |b|); accumulators: rr = sum k1, ii = sum k3, ri = sum k2.
                double asum[TM], bsum[TN], bdif[TN];
#pragma unroll
                for (int t = 0; t < TM; ++t) asum[t] = are[t] + aim[t];
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    bsum[t] = bre[t] + bim[t];
                    bdif[t] = bim[t] - bre[t];
                }
#pragma unroll
                for (int ti = 0; ti < TM; ++ti)
#pragma unroll
                    for (int tj = 0; tj < TN; ++tj) {
                        rr[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bre[tj], asum[ti], rr[ti][tj], 0, 0, 0);
                        ii[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bsum[tj], aim[ti], ii[ti][tj], 0, 0, 0);
                        ri[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bdif[tj], are[ti], ri[ti][tj], 0, 0, 0);
                    }
            } else {
#pragma unroll
                for (int ti = 0; ti < TM; ++ti)
#pragma unroll
                    for (int tj = 0; tj < TN; ++tj) {
                        rr[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bre[tj], are[ti], rr[ti][tj], 0, 0, 0);
                        if constexpr (CX) {                                      // (QIL_GEMM_GAUSS = 0: the four-multiplication form, A/B builds only)
                            ii[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bim[tj], aim[ti], ii[ti][tj], 0, 0, 0);
                            ri[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bim[tj], are[ti], ri[ti][tj], 0, 0, 0);
                            ri[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bre[tj], aim[ti], ri[ti][tj], 0, 0, 0);
                        }
                    }
            }
        }
    };
    if constexpr (PIPE && DEEP) {
        // TWO K tiles in flight (r05): a skinny product streams its long operand once, one row of tiles per workgroup, and
        // with one tile ahead the global-load latency under a full HBM pipe (~3 us) exceeded the MFMA phase it hides behind
        // (~1 us): 32 / 48 / 64 rows x 8192 x 8192 all took 0.47 ms = 2.3 TB/s.  Two register sets alternate; each load has
        // two MFMA phases to land.
        T ra1[EA], rb1[EB];
        if (kbeg < kend) load_tile_into(ra, rb, kbeg);
        if (kbeg + GKT < kend) load_tile_into(ra1, rb1, kbeg + GKT);
        for (long long k0 = kbeg; k0 < kend; k0 += 2 * GKT) {
            store_tile_from(ra, rb, 0, k0);
            __syncthreads();
            if (k0 + 2 * GKT < kend) load_tile_into(ra, rb, k0 + 2 * GKT);
            mfma_tile(0);
            if (k0 + GKT >= kend) break;
            store_tile_from(ra1, rb1, 1, k0 + GKT);
            __syncthreads();
            if (k0 + 3 * GKT < kend) load_tile_into(ra1, rb1, k0 + 3 * GKT);
            mfma_tile(1);
        }
    } else {
        int buf = 0;
        if (PIPE && kbeg < kend) load_tile(kbeg);
        for (long long k0 = kbeg; k0 < kend; k0 += GKT) {
            if (!PIPE) {
                if (k0 > kbeg) __syncthreads();         // everyone is done reading the single buffer
                load_tile(k0);
            }
            store_tile(buf, k0);
            __syncthreads();
            if (PIPE && k0 + GKT < kend) load_tile(k0 + GKT);     // in flight during the MFMAs below
            mfma_tile(buf);
            if (PIPE) buf ^= 1;
        }
    }
    // D fragment of (AB)^T: D'[j][i], i = lane & 15, j = (lane >> 4) + 4 * reg
#pragma unroll
    for (int ti = 0; ti < TM; ++ti)
#pragma unroll
        for (int tj = 0; tj < TN; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long gr = row0 + wr + 16 * ti + l15;
                const long long gc = col0 + wc + 16 * tj + l4 + 4 * r;
                if (gr < m && gc < n) {
                    const long long oc = cmap ? (long long)cmap[gc / cmap_blk] * cmap_blk + gc % cmap_blk : gc;
                    double* cp = reinterpret_cast<double*>(C + gr + ldc * oc);
                    if (subtract) {
                        if (CX) {
                            cp[0] -= rr[ti][tj][r] - ii[ti][tj][r];
                            cp[1] -= QIL_GEMM_GAUSS ? rr[ti][tj][r] + ri[ti][tj][r] : ri[ti][tj][r];
                        } else {
                            cp[0] -= rr[ti][tj][r];
                        }
                    } else if (CX) {
                        cp[0] = rr[ti][tj][r] - ii[ti][tj][r];                   // re = k1 - k3
                        cp[1] = QIL_GEMM_GAUSS ? rr[ti][tj][r] + ri[ti][tj][r] : ri[ti][tj][r];   // im = k1 + k2
                    } else {
                        cp[0] = rr[ti][tj][r];
                    }
                }
            }
}
template <class T, int BM, int BN, int WM, int WN, bool PIPE, bool ARC, bool BKC, int GKT = GK, int DEEP = 0>
struct gemm_mfma_k {
    static constexpr int NT = 256, MINW = (DEEP ? 1 : (BM * BN <= 128 * 128 ? 2 : 1));   // (DEEP: two register sets of staged tiles, no spills)
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        gemm_mfma_body<T, BM, BN, WM, WN, PIPE, ARC, BKC, GKT, DEEP>(b, g, a...);
    }
};

template <class T>
__device__ __forceinline__ void splitk_reduce_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ W, long long cstride, int splits, long long m, long long n,
                              T* __restrict__ C, long long ldc, int subtract) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < m * n;
         t += (long long)gridDim.x * blockDim.x) {
        T acc = W[t];
        for (int z = 1; z < splits; ++z) acc = add_t(acc, W[t + z * cstride]);
        T* cp = C + (t % m) + ldc * (t / m);
        *cp = subtract ? sub_t(*cp, acc) : acc;
    }
}
template <class T>
struct splitk_reduce_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        splitk_reduce_body<T>(b, g, a...);
    }
};

// strided batch (gridDim.y); split-K of a batch needs packed outputs (ldc == m, c_bs == m * n, no cmap)
struct gemm_batch {
    int count = 1;
    long long a_bs = 0, b_bs = 0, c_bs = 0;
    const int* cmap = nullptr;
    int cmap_blk = 1;
    const uint8_t* b_sel = nullptr;
    long long b_sel_step = 0, b_sel_stride = 0;
    int subtract = 0;                   // 1: C <- C - op(A) op(B)  (the projection step of the blocked QR, no temporary)
    int skinny_m = 0;                   // 1: the caller knows op(A) has <= 32 rows and a long n: 32 x 128 output tiles
};

// The tile shapes of the family: (BM, BN, WM, WN, GKT, DEEP).  gemm_plan picks one by its index, gemm_dispatch switches on it.
struct gemm_shape {
    int bm, bn, wm, wn, gkt, deep;
};
enum { GS_32x64_DEEP, GS_48x64_DEEP, GS_32x32, GS_64x64, GS_64x144, GS_128x128, GS_128x64, GS_COUNT };
constexpr gemm_shape GEMM_SHAPES[GS_COUNT] = {
    {32, 64, 16, 32, GK, 1}, {48, 64, 48, 16, GK, 1}, {32, 32, 16, 16, 32, 0}, {64, 64, 32, 32, GK, 0},
    {64, 144, 16, 144, GK, 0}, {128, 128, 64, 64, GK, 0}, {128, 64, 64, 32, GK, 0}};

// which tile shape a product runs on (cx: complex elements)
int gemm_pick_shape(bool cx, long long m, long long n, long long count, int skinny_m) {
    // few output tiles (the 256 x 256 products of the gauge steps: 16 tiles of 64 x 64): a product that leaves most of the chip
    // idle is bound by the K loop of ONE tile on its CU (32 MFMAs per wave and 32-deep K step at 64 x 64, 8 at 32 x 32)
    // (measured, up to 0 / 16 / 32 / 64 tiles of 64 x 64 as 32 x 32 tiles: compress! chi 256 f64 49.5 / 46.2 / 45.6 / 46.1 ms, c64 66.2 /
    // 61.5 / 59.6 / 61.0, chi 512 f64 122.3 / 118.0 / 115.7 / 114.5, c64 165.9 / 151.8 / 148.1 / 142.6, fused apply-and-truncate 147 / 131 / 128 / 129)
    // skinny op(A) (the halves of a bit-sorted coefficient read-out: ~32 queries x 8192 columns x 8192 deep): the product streams
    // its long operand ONCE, one row of tiles.  32 x 64 / 48 x 64 tiles (no rows of padding work; 51 / 59 KB of LDS: 3 / 2
    // workgroups per CU) with TWO K tiles in flight (DEEP).  Measured per 8192 x 8192 complex slice: 64 x 64 tile, one tile ahead
    // 0.47 ms whatever the rows (latency-bound, 2.3 TB/s); 32 x 128 / 48 x 128 one tile ahead the same; 32 x 64 DEEP 0.30 ms
    // (3.5 TB/s), 48 x 64 DEEP 0.43-0.47 ms, 64 x 64 DEEP 0.58 ms -- now proportional to the padded rows (~42 TFLOP/s of real
    // MFMA work, 0.54 of the matrix peak) and independent of the grid size (512 ... 1536 workgroups: equal)
    if (skinny_m && m <= 32 && n >= 128) return GS_32x64_DEEP;
    // ... and 33-48 rows (the larger half of 64 sorted queries is typically 33-40 rows)
    if (skinny_m && m <= 48 && n >= 128) return GS_48x64_DEEP;
    constexpr long long small_tiles = 64;
    // (K step of the small tiles 16 / 32 / 64: compress! chi 256 46.5 / 45.3 / 45.2 ms, chi 512 115.1 / 111.7 / 112.1, exact route 300 / 293 / 294)
    if (((m + 63) / 64) * ((n + 63) / 64) * count <= small_tiles && m >= 32 && n >= 32) return GS_32x32;
    if (cx) return GS_64x64;      // pipelined: equal on big squares, 56 vs 45 TFLOP/s on 64 x 16384 x 8192
    // 97..144 output columns (RSVD sketches with k + p = 133): one 144-wide tile reads A ONCE and pads
    // 133 -> 144 columns instead of 192
    // one 144-wide tile per row panel; 64 rows (one 16 x 144 strip per wave) fit 2 waves/SIMD, 128 rows do not
    // (two K tiles in flight on this tile: 5.9 -> 6.9 ms for 32768 x 133 x 32768, r05 -- it is not latency-bound)
    if (m >= 256 && n > 96 && n <= 144) return GS_64x144;
    // big outputs: 128 x 128 tiles, 4 x 4 MFMA tiles per wave (two fragment reads per MFMA step pair, 64 MFMAs
    // between barriers) at 2 waves/SIMD -- 59 vs 52 TFLOP/s for the 128 x 64 tile at 4096^3
    {
        const long long t128 = ((m + 127) / 128) * ((n + 127) / 128);
        const bool fills = (double)m * (double)n >= 0.85 * 16384.0 * (double)t128;   // little padding in edge tiles
        if (t128 * count >= 512 && fills) return GS_128x128;
    }
    // 128 x 64 tiles only when they still give every CU a workgroup: a product that fills a fraction of the chip is bound by
    // the time of ONE tile on its CU, and a 64 x 64 tile takes half of it
    {
        constexpr long long min_tiles = 128;   // (measured, compress! chi 256 / 512: always 51.9 / 131.1 ms; from 64, 256 or 1024 tiles on: 49.4-50.4 / 123.1 ms)
        const long long t = ((m + 127) / 128) * ((n + 63) / 64) * count;
        if (m >= 256 && t >= min_tiles) return GS_128x64;
    }
    return GS_64x64;
}

// Everything the host decides about one product, from its arguments alone (no context, no device): the tile shape, the staging
// pattern, split-K, the tile order.  gemm_dispatch / gemm_launch switch on the result and decide nothing themselves;
// qil_gemm_plan hands the same struct to the tests.  opA / opB: 0 = N, 1 = T, 2 = H, 3 = conj.  Returns the GS_ index.
int gemm_plan(bool cx, int opA, int opB, long long m, long long n, long long k, long long lda, long long ldb, long long ldc,
              long long count, long long c_bs, bool has_cmap, int skinny_m, qil_gemm_plan_info* p) {
    const int si = gemm_pick_shape(cx, m, n, count, skinny_m);
    const gemm_shape& s = GEMM_SHAPES[si];
    p->bm = s.bm, p->bn = s.bn, p->wm = s.wm, p->wn = s.wn, p->gkt = s.gkt, p->deep = s.deep;
    // op(A)[r, kk] = A[r * a_rs + kk * a_ks];  op(B)[kk, c] = B[kk * b_ks + c * b_cs]
    const bool at = opA == 1 || opA == 2, bt = opB == 1 || opB == 2;
    p->arc = (at ? lda : 1) == 1;
    p->bkc = (bt ? ldb : 1) == 1;
    const long long tiles_m = (m + s.bm - 1) / s.bm, tiles_n = (n + s.bn - 1) / s.bn;
    const long long tiles = tiles_m * tiles_n;
    p->tiles_m = tiles_m, p->tiles_n = tiles_n;
    const bool can_split = count == 1 || (ldc == m && c_bs == m * n && !has_cmap);
    p->can_split = can_split;
    // few output tiles + long K (projections Q^H P, sketches of skinny panels): split K over the chip
    int splits = 1, rule = 0;
    static const long long split_min_k = 1024;   // (measured; 512: exact compress! of the bond-1008 product 572 -> 534 ms, compress! 512 -> 256 330 -> 355 ms)
    // ... and from K = 512 when the output is at most 8 tiles (the CGS2 projections Q^H P of 1008-row complex panels:
    // exact compress! of the bond-1008 product 476 -> 445 ms; splitting every K >= 512 product costs the small chains 5 %)
    if (can_split && tiles * count < 128 && (k >= split_min_k || (k >= 512 && tiles * count <= 8))) {
        splits = (int)std::min<long long>(std::min<long long>(k / 256, 512 / (tiles * count)), 64);
        rule = 1;
    }
    // one to four output tiles (complex: a 64 x 64 tile is 0.85 us of MFMA per 16 k on ITS ONE CU -- the projections and
    // environment products of the truncation chains spend 20-40 us there): slices of 64 k from K = 128 on
    // (measured against no slicing: fused apply-compress 263 -> 244 ms, exact route 439 -> 417 ms)
    if (can_split && tiles * count <= 4 && k >= 128) {
        const int s2 = (int)std::min<long long>(k / 64, 32);
        if (s2 > splits) splits = s2, rule = 2;
    }
    // one wave of workgroups or less and a long K (the encoder's 16384 x 133 x 16384 sketches: 256 tiles): two to four K
    // slices fill the second workgroup slot of every CU (37.7 -> see DESIGN 3.4)
    if (splits < 2 && can_split && tiles * count >= 128 && tiles * count <= 384 && k >= 4096) {
        splits = (int)std::min<long long>(4, (767 / (tiles * count)));
        rule = 3;
    }
    if (splits < 2) splits = 1, rule = 0;
    long long kchunk = k;
    if (splits > 1) {
        kchunk = (((k + splits - 1) / splits) + s.gkt - 1) / s.gkt * s.gkt;
        splits = (int)((k + kchunk - 1) / kchunk);
    }
    p->splits = splits, p->split_rule = rule, p->kchunk = kchunk;
    // narrow outputs: neighbouring workgroups share the same rows of A (served from L2 / Infinity Cache)
    p->col_fastest = tiles_n <= 8 ? 1 : 0;
    // XCD-aware tile order (see the kernel): exact split only, which keeps the map a bijection without a table
    p->xcd = tiles >= 64 && tiles % 8 == 0;
    return si;
}

template <class T, int SI>
int gemm_launch(qil_context* ctx, const qil_gemm_plan_info& p, long long m, long long n, long long k, const T* A, long long a_rs,
                long long a_ks, int conjA, const T* B, long long b_ks, long long b_cs, int conjB, T* C,
                long long ldc, const gemm_batch& bt) {
    constexpr gemm_shape S = GEMM_SHAPES[SI];
    constexpr int BM = S.bm, BN = S.bn, WM = S.wm, WN = S.wn, GKT = S.gkt, DEEP = S.deep;
    constexpr bool PIPE = true;
    constexpr int NP = sizeof(T) == 16 ? 2 : 1;
    constexpr size_t lds = (size_t)(PIPE ? 2 : 1) * NP * GKT * ((BM + GPAD) + (BN + GPAD)) * sizeof(double);
    const long long tiles = p.tiles_m * p.tiles_n;
    const int splits = p.splits;
    long long cstride = 0, c_bs = bt.c_bs;
    T* Cout = C;
    long long ldo = ldc;
    void* wsp = nullptr;
    if (splits > 1) {
        cstride = m * n * bt.count;
        c_bs = m * n;
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(cstride * splits) * sizeof(T), &wsp));
        Cout = static_cast<T*>(wsp);
        ldo = m;
    }
    const int order = p.col_fastest | (p.xcd ? 2 : 0);
#define QIL_GEMM_K(ARCv, BKCv)                                                                                               \
    QIL_TRY((qil_klaunch<gemm_mfma_k<T, BM, BN, WM, WN, PIPE, ARCv, BKCv, GKT, DEEP>>(                                                      \
        ctx, dim3((unsigned)tiles, (unsigned)bt.count, (unsigned)splits), dim3(256), lds, m, n, k, A, a_rs, a_ks, conjA, B, b_ks, \
        b_cs, conjB, Cout, ldo, (long long)p.kchunk, cstride, (int)p.tiles_m, (int)p.tiles_n, order, bt.a_bs, bt.b_bs, c_bs, bt.cmap,  \
        bt.cmap_blk, bt.b_sel, bt.b_sel_step, bt.b_sel_stride, splits > 1 ? 0 : bt.subtract)))
    if (p.arc && p.bkc) QIL_GEMM_K(true, true);
    else if (p.arc) QIL_GEMM_K(true, false);
    else if (p.bkc) QIL_GEMM_K(false, true);
    else QIL_GEMM_K(false, false);
#undef QIL_GEMM_K
    if (splits > 1) {
        // a packed batch reduces as one m x (n * count) matrix
        QIL_TRY((qil_klaunch<splitk_reduce_k<T>>(ctx, dim3((unsigned)std::min<long long>((cstride + 255) / 256, 2048)), dim3(256), 0, (const T*)Cout, cstride, splits, m, n * bt.count, C, ldc, bt.subtract)));
        QIL_HIP(hipGetLastError());
        qil_ctx_free(ctx, wsp);
    }
    return QIL_OK;
}

template <class T>
int gemm_dispatch(qil_context* ctx, int opA, int opB, long long m, long long n, long long k, const T* A,
                  long long lda, const T* B, long long ldb, T* C, long long ldc,
                  const gemm_batch& batch = gemm_batch{}) {
    if (m == 0 || n == 0) return QIL_OK;
    QIL_REQUIRE(opA >= 0 && opA <= 3 && opB >= 0 && opB <= 3, QIL_EINVAL_ARG, "gemm: bad op codes %d, %d", opA, opB);
    // op(A)[r, kk] = A[r * a_rs + kk * a_ks];  op(B)[kk, c] = B[kk * b_ks + c * b_cs]
    const bool at = opA == 1 || opA == 2, bt = opB == 1 || opB == 2;
    const long long a_rs = at ? lda : 1, a_ks = at ? 1 : lda;
    const long long b_ks = bt ? ldb : 1, b_cs = bt ? 1 : ldb;
    const int cA = (opA == 2 || opA == 3) ? 1 : 0, cB = (opB == 2 || opB == 3) ? 1 : 0;
    constexpr bool CX = sizeof(T) == 16;
    qil_gemm_plan_info p;
    const int si = gemm_plan(CX, opA, opB, m, n, k, lda, ldb, ldc, batch.count, batch.c_bs, batch.cmap != nullptr, batch.skinny_m, &p);
#define QIL_GEMM_GO(SI) \
    case SI: return gemm_launch<T, SI>(ctx, p, m, n, k, A, a_rs, a_ks, cA, B, b_ks, b_cs, cB, C, ldc, batch)
    switch (si) {
        QIL_GEMM_GO(GS_32x64_DEEP);
        QIL_GEMM_GO(GS_48x64_DEEP);
        QIL_GEMM_GO(GS_32x32);
        QIL_GEMM_GO(GS_64x64);
    }
    if constexpr (!CX) {            // the wide and the 128-row tiles exist for f64 only
        switch (si) {
            QIL_GEMM_GO(GS_64x144);
            QIL_GEMM_GO(GS_128x128);
            QIL_GEMM_GO(GS_128x64);
        }
    }
#undef QIL_GEMM_GO
    return qil_fail(QIL_EINVAL_ARG, "gemm: no kernel for tile shape %d", si);
}

// ------------------------------------------------------------------ one-sided Jacobi SVD
template <class T>
__device__ __forceinline__ void jacobi_round_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ A, long long lda, long long m,
                                                    T* __restrict__ V, long long ldv, int vrows, int n,
                                                    int npad, int round, double tol,
                                                    int* __restrict__ rotated,
                                                    const double* __restrict__ negligible) {
    __shared__ double red[16];
    const int i = blockIdx.x;
    int p, q;
    if (i == 0) {
        p = npad - 1;
        q = round;
    } else {
        p = (round + i) % (npad - 1);
        q = (round + npad - 1 - i) % (npad - 1);
    }
    if (p >= n || q >= n) return;
    if (p > q) {
        const int t = p;
        p = q;
        q = t;
    }
    T* ap = A + lda * p;
    T* aq = A + lda * q;
    double v[4] = {0, 0, 0, 0};  // alpha, beta, gamma_re, gamma_im
    for (long long r = threadIdx.x; r < m; r += 256) {
        const T x = ap[r], y = aq[r];
        v[0] += abs2_t(x);
        v[1] += abs2_t(y);
        dot_parts(x, y, v[2], v[3]);
    }
    block_sum<4>(v, red);
    if (negligible) {
        const double ng = *negligible;
        if (v[0] < ng || v[1] < ng) return;
    }
    double c, s, pr, pi;
    bool big;
    if (!jacobi_rotation<sizeof(T) == 16>(v[0], v[1], v[2], v[3], tol, c, s, pr, pi, big)) return;
    if (threadIdx.x == 0) {      // plain stores of the same value from every rotating workgroup: no atomics needed
        rotated[0] = 1;
        if (big) rotated[1] = 1;
    }
    for (long long r = threadIdx.x; r < m; r += 256) {
        T x = ap[r], y = aq[r];
        rotate_pair(x, y, c, s, pr, pi);
        ap[r] = x;
        aq[r] = y;
    }
    T* vp = V + ldv * p;
    T* vq = V + ldv * q;
    for (int r = threadIdx.x; r < vrows; r += 256) {
        T x = vp[r], y = vq[r];
        rotate_pair(x, y, c, s, pr, pi);
        vp[r] = x;
        vq[r] = y;
    }
}
template <class T>
struct jacobi_round_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        jacobi_round_body<T>(b, g, a...);
    }
};


// One column pair of an in-LDS block round, handled by one wave.  KM > 0: at most KM elements per lane (m, vrows <= 64 KM);
// all loads of a phase are issued together and the pair is rotated from the registers it was read into for the dot
// products -- with one wave per pair and eight waves per CU the phases are latency chains, and a rolled loop pays one
// LDS round trip per element (1.6 us per inner round).  KM = 0: generic loops.
template <class T, int KM>
__device__ __forceinline__ int block_pair_rotate(T* __restrict__ ap, T* __restrict__ aq, int m, T* __restrict__ vp,
                                                 T* __restrict__ vq, int vrows, int lane, double tol, double ng) {
    double al = 0, be = 0, gr = 0, gi = 0;
    constexpr int KA = KM > 0 ? KM : 1;
    T xs[KA], ys[KA];
    if (KM > 0) {
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int r = lane + 64 * k;
            xs[k] = r < m ? ap[r] : T{};
            ys[k] = r < m ? aq[r] : T{};
        }
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            al += abs2_t(xs[k]);
            be += abs2_t(ys[k]);
            dot_parts(xs[k], ys[k], gr, gi);
        }
    } else {
        for (int r = lane; r < m; r += 64) {
            const T x = ap[r], y = aq[r];
            al += abs2_t(x);
            be += abs2_t(y);
            dot_parts(x, y, gr, gi);
        }
    }
    al = wave_sum(al);
    be = wave_sum(be);
    gr = wave_sum(gr);
    if (sizeof(T) == 16) gi = wave_sum(gi);
    double c, sn, pr, pi;
    bool big;
    if (al < ng || be < ng || !jacobi_rotation<sizeof(T) == 16>(al, be, gr, gi, tol, c, sn, pr, pi, big)) return 0;
    if (KM > 0) {
        T us[KA], ws[KA];
#pragma unroll
        for (int k = 0; k < KA; ++k) {       // V loads go out before the A rotation's arithmetic
            const int r = lane + 64 * k;
            us[k] = r < vrows ? vp[r] : T{};
            ws[k] = r < vrows ? vq[r] : T{};
        }
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int r = lane + 64 * k;
            rotate_pair(xs[k], ys[k], c, sn, pr, pi);
            if (r < m) {
                ap[r] = xs[k];
                aq[r] = ys[k];
            }
        }
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int r = lane + 64 * k;
            rotate_pair(us[k], ws[k], c, sn, pr, pi);
            if (r < vrows) {
                vp[r] = us[k];
                vq[r] = ws[k];
            }
        }
    } else {
        for (int r = lane; r < m; r += 64) {
            T x = ap[r], y = aq[r];
            rotate_pair(x, y, c, sn, pr, pi);
            ap[r] = x;
            aq[r] = y;
        }
        for (int r = lane; r < vrows; r += 64) {
            T x = vp[r], y = vq[r];
            rotate_pair(x, y, c, sn, pr, pi);
            vp[r] = x;
            vq[r] = y;
        }
    }
    return big ? 3 : 1;
}

// One OUTER round of a block tournament for the mid-size regime (97...511 columns), where one launch per scalar
// round costs ~3.9 us for ~1 us of work (every column arrives from another XCD's L2).  Blocks of BB columns are paired
// round-robin; a workgroup stages its 2 BB columns of A and of V in LDS, orthogonalises every CROSS pair of the two
// blocks (BB inner rounds of BB disjoint pairs, one wave per pair) -- or, in the first outer round of a sweep, every
// pair among the 2 BB columns, which also covers the pairs inside each block once per sweep -- and writes the columns
// back.  A sweep is nb - 1 launches instead of n - 1.
template <class T, int BB>
__device__ __forceinline__ void jacobi_block_round_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ A, long long lda, int m,
                                                              T* __restrict__ V, long long ldv, int vrows, int n, int nb,
                                                              int round, int all_pairs, double tol,
                                                              int* __restrict__ rotated,
                                                              const double* __restrict__ negligible) {
    constexpr int W = 2 * BB;
    extern __shared__ __attribute__((aligned(16))) char jb_smem[];
    const int la = m | 1, lv = vrows | 1;
    T* As = reinterpret_cast<T*>(jb_smem);
    T* Vs = As + (size_t)la * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int P, Q;
    {
        const int i = blockIdx.x;
        if (i == 0) {
            P = nb - 1;
            Q = round;
        } else {
            P = (round + i) % (nb - 1);
            Q = (round + nb - 1 - i) % (nb - 1);
        }
        if (P > Q) {
            const int t = P;
            P = Q;
            Q = t;
        }
    }
    auto gcol = [&](int k) { return (k < BB ? P * BB + k : Q * BB + (k - BB)); };
    if (P * BB >= n) return;                               // both blocks are padding
    // staging: every wave owns two of the 2 BB columns (NT / 64 = BB waves), lanes stride the rows -- coalesced, no
    // index division, eight independent loads in flight per thread (a rolled copy loop waits out one L2 / fabric round
    // trip per element, which costs more than the rotations)
    const int kc0 = wave, kc1 = wave + BB;
    const int gc0 = gcol(kc0), gc1 = gcol(kc1);
    auto stage = [&](const T* __restrict__ G, long long ldg, int rws, T* __restrict__ S, int lds_) {
        const T* s0 = G + ldg * gc0;
        const T* s1 = G + ldg * gc1;
        T* d0 = S + (size_t)lds_ * kc0;
        T* d1 = S + (size_t)lds_ * kc1;
        for (int r0 = lane; r0 < rws; r0 += 256) {
            T t0[4], t1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + 64 * u;
                t0[u] = (gc0 < n && r < rws) ? s0[r] : T{};
                t1[u] = (gc1 < n && r < rws) ? s1[r] : T{};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + 64 * u;
                if (r < rws) {
                    d0[r] = t0[u];
                    d1[r] = t1[u];
                }
            }
        }
    };
    stage(A, lda, m, As, la);
    stage(V, ldv, vrows, Vs, lv);
    __syncthreads();
    const double ng = negligible ? *negligible : 0.0;
    int flags = 0;
    const int nin = all_pairs ? W - 1 : BB;
    for (int t = 0; t < nin; ++t) {
        int p, q;
        if (all_pairs) {
            if (wave == 0) {
                p = W - 1;
                q = t;
            } else {
                p = (t + wave) % (W - 1);
                q = (t + W - 1 - wave) % (W - 1);
            }
            if (p > q) {
                const int t2 = p;
                p = q;
                q = t2;
            }
        } else {
            p = wave;
            q = BB + (wave + t) % BB;
        }
        if (gcol(p) < n && gcol(q) < n) {
            T* ap = As + (size_t)la * p;
            T* aq = As + (size_t)la * q;
            T* vp = Vs + (size_t)lv * p;
            T* vq = Vs + (size_t)lv * q;
            const int mx = max(m, vrows);
            if (mx <= 256) flags |= block_pair_rotate<T, 4>(ap, aq, m, vp, vq, vrows, lane, tol, ng);
            else if (mx <= 512) flags |= block_pair_rotate<T, 8>(ap, aq, m, vp, vq, vrows, lane, tol, ng);
            else flags |= block_pair_rotate<T, 0>(ap, aq, m, vp, vq, vrows, lane, tol, ng);
        }
        __syncthreads();
    }
    if (lane == 0 && flags) {        // plain stores of the same value from every rotating wave
        rotated[0] = 1;
        if (flags & 2) rotated[1] = 1;
    }
    auto unstage = [&](T* __restrict__ G, long long ldg, int rws, const T* __restrict__ S, int lds_) {
        if (gc0 < n) {
            T* d = G + ldg * gc0;
            const T* sp = S + (size_t)lds_ * kc0;
            for (int r = lane; r < rws; r += 64) d[r] = sp[r];
        }
        if (gc1 < n) {
            T* d = G + ldg * gc1;
            const T* sp = S + (size_t)lds_ * kc1;
            for (int r = lane; r < rws; r += 64) d[r] = sp[r];
        }
    };
    unstage(A, lda, m, As, la);
    unstage(V, ldv, vrows, Vs, lv);
}
template <class T, int BB>
struct jacobi_block_round_k {
    static constexpr int NT = 64 * BB, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        jacobi_block_round_body<T, BB>(b, g, a...);
    }
};

// MODE 1: A and V staged in LDS for the whole iteration; MODE 2: only A in LDS, V in global memory (complex operands of
// 2 chi x chi sites with chi ~ 64: A fits the CU's LDS, A and V together do not) -- the dot products and the rotation
// of A, which every round's critical path waits for, still run out of LDS.
template <class T, int MODE>
__device__ __forceinline__ void jacobi_fused_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ A, long long lda, int m,
                                                     T* __restrict__ V, long long ldv, int n, double tol,
                                                     int max_sweeps, double* __restrict__ norms, double negl_rel) {
    extern __shared__ __attribute__((aligned(16))) char jf_smem[];
    __shared__ int s_rot;
    __shared__ double s_fro[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = 16;
    // odd leading dimension (in doubles): column pairs start on different banks
    const int la = m | 1;
    T* Aw = reinterpret_cast<T*>(jf_smem);
    T* Vw = V;
    int lv = (int)ldv;
    if (MODE == 1) {
        lv = n | 1;
        Vw = Aw + (size_t)la * n;
    }
    for (int t = tid; t < m * n; t += 1024) Aw[(t % m) + la * (t / m)] = A[(t % m) + lda * (t / m)];
    for (int t = tid; t < n * n; t += 1024) {
        const int r = t % n, c = t / n;
        T v{};
        if (r == c) reinterpret_cast<double*>(&v)[0] = 1.0;
        Vw[r + lv * c] = v;
    }
    __threadfence_block();
    __syncthreads();
    double negligible = 0.0;
    if (negl_rel > 0.0) {
        double f = 0;
        for (int t = tid; t < m * n; t += 1024) f += abs2_t(Aw[(t % m) + (long long)la * (t / m)]);
        f = wave_sum(f);
        if (lane == 0) s_fro[wave] = f;
        __syncthreads();
        f = 0;
        for (int w = 0; w < 16; ++w) f += s_fro[w];
        negligible = negl_rel * f;
    }
    // DPP lane-group exec masks must be uniform per group: the `continue`s above are per pair = per group
    if (m <= 128)
        jacobi_sweeps<T, 16>(Aw, la, m, Vw, lv, n, tol, max_sweeps, &s_rot, negligible);
    else
        jacobi_sweeps<T, 64>(Aw, la, m, Vw, lv, n, tol, max_sweeps, &s_rot, negligible);
    for (int j = wave; j < n; j += NW) {
        const T* a = Aw + la * j;
        double v = 0;
        for (int r = lane; r < m; r += 64) v += abs2_t(a[r]);
        v = wave_sum(v);
        if (lane == 0) norms[j] = sqrt(v);
    }
    __syncthreads();
    for (int t = tid; t < m * n; t += 1024) A[(t % m) + lda * (t / m)] = Aw[(t % m) + la * (t / m)];
    if (MODE == 1)
        for (int t = tid; t < n * n; t += 1024) V[(t % n) + ldv * (t / n)] = Vw[(t % n) + lv * (t / n)];
}
template <class T, int MODE>
struct jacobi_fused_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        jacobi_fused_body<T, MODE>(b, g, a...);
    }
};

template <class T>
__device__ __forceinline__ void col_norms_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ A, long long lda, long long m,
                                                 double* __restrict__ out) {
    __shared__ double red[4];
    const T* a = A + lda * blockIdx.x;
    double v[1] = {0};
    for (long long r = threadIdx.x; r < m; r += 256) v[0] += abs2_t(a[r]);
    block_sum<1>(v, red);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt(v[0]);
}
template <class T>
struct col_norms_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        col_norms_body<T>(b, g, a...);
    }
};

template <class T>
__device__ __forceinline__ void set_identity_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ V, long long ldv, int n) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < (long long)n * n;
         t += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(t % n), c = (int)(t / n);
        T v{};
        if (r == c) reinterpret_cast<double*>(&v)[0] = 1.0;
        V[r + ldv * c] = v;
    }
}
template <class T>
struct set_identity_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        set_identity_body<T>(b, g, a...);
    }
};

// dst[:, j] = src[:, perm[j]] * scale[j]   (conjT = 0)   or   dst[j, i] = conj(src[i, perm[j]]) * scale[j]
template <class T>
__device__ __forceinline__ void gather_cols_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ src, long long lds_, long long rows,
                            const int* __restrict__ perm, const double* __restrict__ scale, T* __restrict__ dst,
                            long long ldd, int r0, int conjT) {
    const long long total = rows * r0;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long i = t % rows;
        const int j = (int)(t / rows);
        T v = src[i + lds_ * perm[j]];
        if (scale) v = scale_t(v, scale[j]);
        if (conjT)
            dst[j + ldd * i] = conj_t(v);
        else
            dst[i + ldd * j] = v;
    }
}
template <class T>
struct gather_cols_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        gather_cols_body<T>(b, g, a...);
    }
};

template <class T, bool CONJ = true>
__device__ __forceinline__ void conj_transpose_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ A, long long lda, long long m, long long n,
                               T* __restrict__ At, long long ldt) {
    const long long total = m * n;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long j = t % n, i = t / n;  // write-coalesced
        const T v = A[i + lda * j];
        At[j + ldt * i] = CONJ ? conj_t(v) : v;
    }
}
template <class T, bool CONJ = true>
struct conj_transpose_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        conj_transpose_body<T, CONJ>(b, g, a...);
    }
};

// Whole CGS2 QR in ONE launch of ONE 1024-thread workgroup (small/medium panels).  Per column, two
// project/subtract passes then normalisation.  The projections c[i] = q_i^H y for ALL previous columns
// are accumulated together: every thread owns rows (tid, tid+1024, ...) and keeps up to 16 partial dot
// products in registers, so each pass is one sweep over the rows with 1024 loads in flight, followed by
// one DPP/LDS reduction -- not one latency-bound loop per previous column.
// Numerically dependent columns: a column whose residual after the projections is below 1e-13 of its
// ORIGINAL norm (`ref_norm[j]` if given -- the blocked driver measures it before its GEMM projections --
// else the norm on entry) carries nothing but rounding noise.  Normalising that noise would produce a unit
// vector that is NOT orthogonal to the previous ones ("twice is enough" does not hold for pure noise), and
// every later projection through it would be wrong.  Such a column is dropped as a ZERO column with a zero
// R diagonal: A = Q R still holds and Q^H Q is the projector on the numerical range.
// Chunk mode (chunk_rows > 0, first level of the tall-skinny tree below): workgroup c factors rows
// [c*chunk_rows, ...) on its own and writes its n x n triangle to rows [c*n, (c+1)*n) of a stacked R.
// LDS = true: the workgroup's rows x n slice is staged in LDS (odd leading dimension) for the whole factorisation and
// written back at the end -- every phase of every column is a dependent round trip to wherever the slice lives, and
// a 512 x 55 sketch out of L2 took 22 us per column (1.2 ms per QR, 3/4 of an n = 24 RSVD encode).
template <class T, bool LDS>
__device__ __forceinline__ void gs_fused_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ Ag, long long ldg, long long mtot, int n,
                                                 T* __restrict__ R, long long ldr,
                                                 const double* __restrict__ ref_norm, long long chunk_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* c = reinterpret_cast<T*>(smem_raw);                 // n entries
    __shared__ double red[16][36];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int m = (int)mtot;
    if (chunk_rows > 0) {
        const long long r0 = blockIdx.x * chunk_rows;
        Ag += r0;
        m = (int)min(chunk_rows, mtot - r0);
        if (R) R += (long long)blockIdx.x * n;
    }
    constexpr int NW = 16, CH = 16;
    constexpr int NC = sizeof(T) == 16 ? 2 : 1;
    T* A = Ag;
    long long lda = ldg;
    T* csum = c + (n + (n & 1));                           // first-pass projections (LDS mode only)
    if (LDS) {
        A = csum + (n + (n & 1));
        lda = m | 1;
        // one wave per column, lanes stride the rows (coalesced, no index division), four loads in flight per lane
        for (int k = wave; k < n; k += NW) {
            const T* src = Ag + ldg * k;
            T* dst = A + lda * k;
            for (int r0 = lane; r0 < m; r0 += 256) {
                T t4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t4[u] = r0 + 64 * u < m ? src[r0 + 64 * u] : T{};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (r0 + 64 * u < m) dst[r0 + 64 * u] = t4[u];
            }
        }
    }
    if (R)
        for (int t = tid; t < n * n; t += 1024) R[(t % n) + ldr * (t / n)] = T{};
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        T* y = A + lda * j;
        double nrm0;
        if (ref_norm) {
            nrm0 = ref_norm[j];
        } else {
            double v0 = 0;
            for (int r = tid; r < m; r += 1024) v0 += abs2_t(y[r]);
            v0 = wave_sum(v0);
            if (lane == 0) red[wave][33] = v0;
            __syncthreads();
            double t0 = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t0 += red[w][33];
            nrm0 = sqrt(t0);
            __syncthreads();
        }
        for (int pass = 0; pass < 2 && j > 0 && LDS; ++pass) {
            // slice in LDS: one previous column per lane group (a 16-lane DPP row for short columns, a wave otherwise),
            // every dot product a short independent chain; R is written once, after the second pass
            if (m <= 256) {
                const int l16 = tid & 15;
                for (int i = tid >> 4; i < j; i += 64) {
                    const T* qi = A + lda * i;
                    double a0 = 0, a1 = 0;
                    for (int r = l16; r < m; r += 16) dot_parts(qi[r], y[r], a0, a1);
                    a0 = row16_sum(a0);
                    if (NC == 2) a1 = row16_sum(a1);
                    if (l16 == 0) {
                        T out{};
                        reinterpret_cast<double*>(&out)[0] = a0;
                        if (NC == 2) reinterpret_cast<double*>(&out)[1] = a1;
                        c[i] = out;
                    }
                }
            } else {
                for (int i = wave; i < j; i += NW) {
                    const T* qi = A + lda * i;
                    double a0 = 0, a1 = 0;
                    for (int r = lane; r < m; r += 64) dot_parts(qi[r], y[r], a0, a1);
                    a0 = wave_sum(a0);
                    if (NC == 2) a1 = wave_sum(a1);
                    if (lane == 0) {
                        T out{};
                        reinterpret_cast<double*>(&out)[0] = a0;
                        if (NC == 2) reinterpret_cast<double*>(&out)[1] = a1;
                        c[i] = out;
                    }
                }
            }
            __syncthreads();
            for (int r = tid; r < m; r += 1024) {
                // four independent chains, loads of a group issued together (a rolled single chain waits out one LDS
                // round trip per previous column)
                T s0{}, s1{}, s2{}, s3{};
                int i = 0;
                for (; i + 4 <= j; i += 4) {
                    const T a0 = A[r + lda * i], a1 = A[r + lda * (i + 1)], a2 = A[r + lda * (i + 2)],
                            a3 = A[r + lda * (i + 3)];
                    s0 = fma_t(a0, c[i], s0);
                    s1 = fma_t(a1, c[i + 1], s1);
                    s2 = fma_t(a2, c[i + 2], s2);
                    s3 = fma_t(a3, c[i + 3], s3);
                }
                for (; i < j; ++i) s0 = fma_t(A[r + lda * i], c[i], s0);
                y[r] = sub_t(y[r], add_t(add_t(s0, s1), add_t(s2, s3)));
            }
            for (int i = tid; i < j; i += 1024) {
                if (pass == 0) csum[i] = c[i];
                else if (R) R[i + ldr * j] = add_t(csum[i], c[i]);
            }
            __syncthreads();
        }
        for (int pass = 0; pass < 2 && j > 0 && !LDS; ++pass) {
            for (int i0 = 0; i0 < j; i0 += CH) {
                const int nc = min(CH, j - i0);
                double acc[CH][2];
#pragma unroll
                for (int i = 0; i < CH; ++i) acc[i][0] = acc[i][1] = 0.0;
                for (int r = tid; r < m; r += 1024) {
                    const T yv = y[r];
#pragma unroll
                    for (int i = 0; i < CH; ++i)
                        if (i < nc) dot_parts(A[r + lda * (i0 + i)], yv, acc[i][0], acc[i][1]);
                }
#pragma unroll
                for (int i = 0; i < CH; ++i)
                    if (i < nc) {
                        const double s0 = wave_sum(acc[i][0]);
                        if (lane == 0) red[wave][2 * i] = s0;
                        if (NC == 2) {
                            const double s1 = wave_sum(acc[i][1]);
                            if (lane == 0) red[wave][2 * i + 1] = s1;
                        }
                    }
                __syncthreads();
                if (tid < nc) {
                    double sr = 0, si = 0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        sr += red[w][2 * tid];
                        if (NC == 2) si += red[w][2 * tid + 1];
                    }
                    T out{};
                    reinterpret_cast<double*>(&out)[0] = sr;
                    if (NC == 2) reinterpret_cast<double*>(&out)[1] = si;
                    c[i0 + tid] = out;
                }
                __syncthreads();
            }
            for (int r = tid; r < m; r += 1024) {
                T acc = y[r];
                for (int i = 0; i < j; ++i) acc = sub_t(acc, fma_t(A[r + lda * i], c[i], T{}));
                y[r] = acc;
            }
            if (R)
                for (int i = tid; i < j; i += 1024) R[i + ldr * j] = add_t(R[i + ldr * j], c[i]);
            __threadfence_block();
            __syncthreads();
        }
        double v = 0;
        for (int r = tid; r < m; r += 1024) v += abs2_t(y[r]);
        v = wave_sum(v);
        if (lane == 0) red[wave][32] = v;
        __syncthreads();
        double tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += red[w][32];
        const double nrm = sqrt(tot);
        const bool dep = !(nrm > 1e-13 * nrm0);
        const double inv = dep ? 0.0 : 1.0 / nrm;
        for (int r = tid; r < m; r += 1024) y[r] = scale_t(y[r], inv);
        if (R && tid == 0) {
            T out{};
            reinterpret_cast<double*>(&out)[0] = dep ? 0.0 : nrm;
            R[j + ldr * j] = out;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (LDS)
        for (int k = wave; k < n; k += NW) {
            T* dst = Ag + ldg * k;
            const T* src = A + lda * k;
            for (int r = lane; r < m; r += 64) dst[r] = src[r];
        }
}
template <class T, bool LDS>
struct gs_fused_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        gs_fused_body<T, LDS>(b, g, a...);
    }
};

// ------------------------------------------------------------------ Householder panel (in LDS)
// Thin QR of one panel P (m x b, b <= 32) resident in LDS, the intra-panel step of the blocked QR below (r02; it
// replaces the CGS2 panel kernel gs_fused there).  Householder reflectors (every wave updates the trailing columns it
// owns, two at a time; the owner of the NEXT column updates that one first and derives its reflector while the others
// are still updating: one barrier per column), explicit Q formed barrier-free (columns held in registers, two per wave at
// a time), positive real diagonal of R by a column phase.  Staircase form for numerically dependent columns -- residual below 1e-13 of
// the column's ORIGINAL norm (ref_norm: measured by the blocked driver before its projections): such a column gets no
// reflector and no row, comes out as a ZERO column of Q with a zero row of R, and P = Q R still holds (its components
// along the earlier reflectors' rows stay in R) -- the contract the CGS2 kernel established for rank-deficient
// operands (product bonds before truncation, sketches wider than the rank).
template <class T>
__device__ __forceinline__ T hh_mul_conj(T a, T b);      // conj(a) * b
template <>
__device__ __forceinline__ double hh_mul_conj<double>(double a, double b) { return a * b; }
template <>
__device__ __forceinline__ c64 hh_mul_conj<c64>(c64 a, c64 b) {
    return c64{a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
__device__ __forceinline__ double hh_cmul(double a, double b) { return a * b; }
__device__ __forceinline__ c64 hh_cmul(c64 a, c64 b) { return c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ double hh_wave_sum(double v) { return wave_sum(v); }
__device__ __forceinline__ c64 hh_wave_sum(c64 v) {     // both parts in one reduction tree; every call site has the whole wave active
    wave_sum2(v.re, v.im);
    return v;
}

__device__ __forceinline__ void hh_wave_sum_pair(double& a, double& b) { wave_sum2(a, b); }
__device__ __forceinline__ void hh_wave_sum_pair(c64& a, c64& b) {
    wave_sum2(a.re, a.im);
    wave_sum2(b.re, b.im);
}

// Row predicates are kept out of the instruction stream (a select around a load becomes a branch with a wait inside, one
// per element): every column has a zero SINK row m behind its data, lanes beyond the matrix read and write that row, and
// the staircase mask enters as a multiplication by 0 / 1 -- the update y -= f x then rewrites the rows above the staircase
// with the values they already hold.
template <class T, int KM>
constexpr int hh_panel_waves() { return KM * (int)(sizeof(T) / 8) > 18 ? 8 : 16; }   // long columns: 256 registers per lane

template <class T, int KM, bool PROF = false>
__device__ __forceinline__ void hh_panel_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ P, long long lda, int m, int b,
                                                                         T* __restrict__ R, long long ldr,
                                                                         const double* __restrict__ ref_norm,
                                                                         long long* __restrict__ prof = nullptr) {
    constexpr int NW = hh_panel_waves<T, KM>();
    long long tp0 = 0, tp1 = 0, tp2 = 0, tp3 = 0;          // PROF: s_memtime stamps (tools/micro/hh_panel_cost.hip)
    if (PROF) tp0 = __builtin_amdgcn_s_memtime();
    constexpr bool PAIR = KM * (int)(sizeof(T) / 8) <= 8;   // register budget: 128 per lane with 16 waves (longer columns would spill)
    extern __shared__ __attribute__((aligned(16))) char hp_smem[];
    const int la = (m + 1) | 1;
    T* Ps = reinterpret_cast<T*>(hp_smem);
    double* kap = reinterpret_cast<double*>(Ps + (size_t)la * b);       // b: kappa of column j's reflector (0: none)
    double* dia = kap + 32;                                              // b: |R_jj|
    double* refn = dia + 32;                                             // b: reference norms
    T* pha = reinterpret_cast<T*>(refn + 32);                            // b: column phase making R_jj real positive
    T* dif = pha + 32;                                                   // b: first entry of u_j
    int* rowof = reinterpret_cast<int*>(dif + 32);                       // b: staircase row of column j, -1 = dependent
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto rowc = [&](int u) { return min(lane + 64 * u, m); };          // this lane's rows (sink row m beyond the matrix)
    // stage: wave w owns columns w, w + 16 (all loads of a column in flight)
    for (int c = wave; c < b; c += NW) {
        const T* src = P + lda * c;
        T t0[KM];
#pragma unroll
        for (int u = 0; u < KM; ++u) t0[u] = scale_t(src[rowc(u) < m ? rowc(u) : 0], rowc(u) < m ? 1.0 : 0.0);
        double nn = 0;
#pragma unroll
        for (int u = 0; u < KM; ++u) {
            Ps[rowc(u) + (size_t)la * c] = t0[u];                         // the sink row receives 0
            nn += abs2_t(t0[u]);
        }
        nn = wave_sum(nn);
        if (lane == 0) refn[c] = ref_norm ? ref_norm[c] : sqrt(nn);
    }
    __syncthreads();
    if (PROF) tp1 = __builtin_amdgcn_s_memtime();
    // Reflector of column jn from the column's current values yv (the calling wave's registers; the staircase entry is read
    // back from LDS).  ONE wave runs this -- the owner of the column, right after it has applied the previous reflector to it
    // and while the other waves are still updating theirs; everybody picks kappa, the first entry of u and the staircase row
    // up after the barrier.  (Every wave deriving every reflector redundantly made the column loop ISSUE-bound: four waves
    // per SIMD x ~90 instructions of reductions and reciprocal square roots per column, 3 200 cycles per column measured
    // with tools/micro/hh_panel_cost.hip whatever the column length.)
    auto derive = [&](int jn, int rrn, const T(&yv)[KM]) {
        double s2 = 0;
#pragma unroll
        for (int u = 0; u < KM; ++u) s2 += (rowc(u) > rrn && rowc(u) < m) ? abs2_t(yv[u]) : 0.0;
        s2 = wave_sum(s2);
        const T alpha = Ps[(rrn < m ? rrn : m) + (size_t)la * jn];
        // the column's norm, |alpha| and kappa sit on the dependent chain of every column: reciprocal square roots and
        // reciprocals with one Newton step (1-2 ulp) instead of the IEEE sqrt / divide sequences (~4 x 30 instructions)
        const double a2 = abs2_t(alpha);
        const double t2 = a2 + s2;
        const double nrm = t2 > 0.0 ? t2 * rsqrt_refined(t2) : 0.0;
        const double rn = refn[jn];
        const bool dep = rrn >= m || !(nrm > 1e-13 * rn) || rn == 0.0;
        double kappa = 0.0, absa = 0.0;
        T pa{}, diff{};
        if (!dep) {
            // phase of alpha (1 if alpha == 0): beta = -phase * nrm, u_r = alpha - beta = phase (|alpha| + nrm)
            reinterpret_cast<double*>(&pa)[0] = 1.0;
            if (a2 > 0.0) {
                const double ra = rsqrt_refined(a2);
                absa = a2 * ra;
                pa = scale_t(alpha, ra);
            }
            diff = scale_t(pa, absa + nrm);
            kappa = rcp_refined(nrm * (nrm + absa));
        }
        if (lane == 0) {
            kap[jn] = kappa;
            rowof[jn] = dep ? -1 : rrn;
            if (!dep) {
                dia[jn] = nrm;
                pha[jn] = scale_t(pa, -1.0);                 // beta / |beta|
                dif[jn] = diff;
                Ps[rrn + (size_t)la * jn] = diff;            // first entry of u_jn (nobody reads alpha again)
            }
        }
    };
    if (wave == 0) {
        T y0[KM];
#pragma unroll
        for (int u = 0; u < KM; ++u) y0[u] = Ps[rowc(u)];
        derive(0, 0, y0);
    }
    __syncthreads();
    int rr = 0;                                            // staircase row: identical in every thread
    for (int j = 0; j < b; ++j) {
        const T* x = Ps + (size_t)la * j;
        const double kappa = kap[j];
        const bool dep = rowof[j] < 0;
        const int rrn = dep ? rr : rr + 1;                 // staircase row of the next column
        T diff{};
        if (!dep) diff = dif[j];
        T xs[KM];
#pragma unroll
        for (int u = 0; u < KM; ++u) xs[u] = scale_t(x[rowc(u)], (rowc(u) > rr && rowc(u) < m) ? 1.0 : 0.0);
        int c = j + 1 + ((wave - (j + 1)) % NW + NW) % NW;
        if (c == j + 1 && c < b) {                         // owner of the next column: update it first, then its reflector
            T* y = Ps + (size_t)la * c;
            T ys[KM];
#pragma unroll
            for (int u = 0; u < KM; ++u) ys[u] = y[rowc(u)];
            if (!dep) {
                const T yr = y[rr];
                T w{};
#pragma unroll
                for (int u = 0; u < KM; ++u) w = add_t(w, hh_mul_conj(xs[u], ys[u]));
                w = hh_wave_sum(w);
                w = add_t(w, hh_mul_conj(diff, yr));
                const T f = scale_t(w, kappa);
#pragma unroll
                for (int u = 0; u < KM; ++u) {
                    ys[u] = sub_t(ys[u], hh_cmul(f, xs[u]));
                    y[rowc(u)] = ys[u];
                }
                if (lane == 0) y[rr] = sub_t(yr, hh_cmul(f, diff));
            }
            derive(c, rrn, ys);
            c += NW;
        }
        if (!dep) {
            if constexpr (PAIR) {
                // two of this wave's trailing columns at a time: one set of LDS round trips and ONE reduction tree for
                // both dot products instead of two dependent passes
                for (; c + NW < b; c += 2 * NW) {
                    T* y0 = Ps + (size_t)la * c;
                    T* y1 = y0 + (size_t)la * NW;
                    T ya[KM], yb[KM];
#pragma unroll
                    for (int u = 0; u < KM; ++u) {
                        ya[u] = y0[rowc(u)];
                        yb[u] = y1[rowc(u)];
                    }
                    const T ra = y0[rr], rb = y1[rr];
                    T wa{}, wb{};
#pragma unroll
                    for (int u = 0; u < KM; ++u) {
                        wa = add_t(wa, hh_mul_conj(xs[u], ya[u]));
                        wb = add_t(wb, hh_mul_conj(xs[u], yb[u]));
                    }
                    hh_wave_sum_pair(wa, wb);
                    wa = add_t(wa, hh_mul_conj(diff, ra));
                    wb = add_t(wb, hh_mul_conj(diff, rb));
                    const T fa = scale_t(wa, kappa), fb = scale_t(wb, kappa);
#pragma unroll
                    for (int u = 0; u < KM; ++u) {
                        y0[rowc(u)] = sub_t(ya[u], hh_cmul(fa, xs[u]));
                        y1[rowc(u)] = sub_t(yb[u], hh_cmul(fb, xs[u]));
                    }
                    if (lane == 0) {
                        y0[rr] = sub_t(ra, hh_cmul(fa, diff));
                        y1[rr] = sub_t(rb, hh_cmul(fb, diff));
                    }
                }
            }
            for (; c < b; c += NW) {
                T* y = Ps + (size_t)la * c;
                T ys[KM];
#pragma unroll
                for (int u = 0; u < KM; ++u) ys[u] = y[rowc(u)];
                const T yr = y[rr];
                T w{};
#pragma unroll
                for (int u = 0; u < KM; ++u) w = add_t(w, hh_mul_conj(xs[u], ys[u]));      // xs is 0 above the staircase
                w = hh_wave_sum(w);
                w = add_t(w, hh_mul_conj(diff, yr));
                const T f = scale_t(w, kappa);
#pragma unroll
                for (int u = 0; u < KM; ++u) y[rowc(u)] = sub_t(ys[u], hh_cmul(f, xs[u]));
                if (lane == 0) y[rr] = sub_t(yr, hh_cmul(f, diff));
            }
        }
        __syncthreads();
        rr = rrn;
    }
    __syncthreads();
    if (PROF) tp2 = __builtin_amdgcn_s_memtime();
    // R block (b x b): row jj = conj(phase_jj) * staircase row rowof[jj]; zero rows for dependent columns
    if (R)
        for (int t = tid; t < b * b; t += 64 * NW) {
            const int jj = t % b, c = t / b;
            T v{};
            const int ro = rowof[jj];
            if (ro >= 0 && c >= jj) {
                if (c == jj) reinterpret_cast<double*>(&v)[0] = dia[jj];
                else v = hh_mul_conj(pha[jj], Ps[ro + (size_t)la * c]);
            }
            R[jj + ldr * c] = v;
        }
    // the reflectors, cleaned for the Q loop below: zeros above the staircase row (those entries were R's, just written
    // out) and in dependent columns, so that the loop reads them without a mask
    __syncthreads();
    for (int c = wave; c < b; c += NW) {
        const int ro = rowof[c];
        T* x = Ps + (size_t)la * c;
        if (ro < 0) {
#pragma unroll
            for (int u = 0; u < KM; ++u) x[rowc(u)] = T{};
        } else if (lane < ro) {
            x[lane] = T{};                                   // ro <= c < 32
        }
    }
    __syncthreads();
    if (PROF) tp3 = __builtin_amdgcn_s_memtime();
    // explicit Q: column c = phase_c * H_{j0} ... H_{jk} e_{rowof[c]} over the independent columns j <= c, last first.
    // (A compact-WY formation -- Gram matrix by MFMA, T by back substitution, Q = E - V T W by MFMA tiles -- was built and
    // measured slower: the 32 dependent rows of the triangular solve cost ~650 cycles each between barriers, 39 k cycles
    // against this loop's 34 k for a 256 x 32 f64 panel, 73 k against 79 k for a complex one.)
    int cq = wave;
    if constexpr (PAIR) {
        // columns c and c + NW of this wave together: the reflectors j in (c, c + NW] act on the second one only, the
        // rest on both with one LDS read of the reflector and one reduction tree
        for (; cq + NW < b; cq += 2 * NW) {
            const int c0 = cq, c1 = cq + NW;
            const int r0 = rowof[c0], r1 = rowof[c1];
            T qa[KM], qb[KM];
#pragma unroll
            for (int u = 0; u < KM; ++u) {
                qa[u] = T{};
                qb[u] = T{};
                if (lane + 64 * u == r0) reinterpret_cast<double*>(&qa[u])[0] = 1.0;
                if (lane + 64 * u == r1) reinterpret_cast<double*>(&qb[u])[0] = 1.0;
            }
            for (int j = c1; j >= 0; --j) {
                const double kappa = kap[j];
                const int rj = rowof[j];
                if (kappa == 0.0 || rj < 0) continue;
                const T* x = Ps + (size_t)la * j;
                T xs[KM];
                T wa{}, wb{};
#pragma unroll
                for (int u = 0; u < KM; ++u) {
                    xs[u] = x[rowc(u)];
                    wa = add_t(wa, hh_mul_conj(xs[u], qa[u]));
                    wb = add_t(wb, hh_mul_conj(xs[u], qb[u]));
                }
                hh_wave_sum_pair(wa, wb);
                const T fa = scale_t(wa, (j <= c0 && r0 >= 0) ? kappa : 0.0), fb = scale_t(wb, r1 >= 0 ? kappa : 0.0);
#pragma unroll
                for (int u = 0; u < KM; ++u) {
                    qa[u] = sub_t(qa[u], hh_cmul(fa, xs[u]));
                    qb[u] = sub_t(qb[u], hh_cmul(fb, xs[u]));
                }
            }
            const T pa = r0 >= 0 ? pha[c0] : T{}, pb = r1 >= 0 ? pha[c1] : T{};
            T* d0 = P + lda * c0;
            T* d1 = P + lda * c1;
#pragma unroll
            for (int u = 0; u < KM; ++u) {
                const int r = lane + 64 * u;
                if (r < m) {
                    d0[r] = r0 >= 0 ? hh_cmul(qa[u], pa) : T{};
                    d1[r] = r1 >= 0 ? hh_cmul(qb[u], pb) : T{};
                }
            }
        }
    }
    for (int c = cq; c < b; c += NW) {
        T* dst = P + lda * c;
        const int ro = rowof[c];
        T q[KM];
#pragma unroll
        for (int u = 0; u < KM; ++u) {
            q[u] = T{};
            if (lane + 64 * u == ro) reinterpret_cast<double*>(&q[u])[0] = 1.0;
        }
        if (ro >= 0)
            for (int j = c; j >= 0; --j) {
                const double kappa = kap[j];
                const int rj = rowof[j];
                if (kappa == 0.0 || rj < 0) continue;
                const T* x = Ps + (size_t)la * j;
                T xs[KM];
                T w{};
#pragma unroll
                for (int u = 0; u < KM; ++u) {
                    xs[u] = x[rowc(u)];
                    w = add_t(w, hh_mul_conj(xs[u], q[u]));
                }
                w = hh_wave_sum(w);
                const T f = scale_t(w, kappa);
#pragma unroll
                for (int u = 0; u < KM; ++u) q[u] = sub_t(q[u], hh_cmul(f, xs[u]));
            }
        const T ph = ro >= 0 ? pha[c] : T{};
#pragma unroll
        for (int u = 0; u < KM; ++u) {
            const int r = lane + 64 * u;
            if (r < m) dst[r] = ro >= 0 ? hh_cmul(q[u], ph) : T{};
        }
    }
    if (PROF) {
        __syncthreads();
        if (tid == 0) {
            const long long tp4 = __builtin_amdgcn_s_memtime();
            atomicAdd((unsigned long long*)prof + 0, (unsigned long long)(tp1 - tp0));
            atomicAdd((unsigned long long*)prof + 1, (unsigned long long)(tp2 - tp1));
            atomicAdd((unsigned long long*)prof + 2, (unsigned long long)(tp3 - tp2));
            atomicAdd((unsigned long long*)prof + 3, (unsigned long long)(tp4 - tp3));
            atomicAdd((unsigned long long*)prof + 4, 1ull);
        }
    }
}
template <class T, int KM, bool PROF = false>
struct hh_panel_k {
    static constexpr int NT = (64 * hh_panel_waves<T, KM>()), MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        hh_panel_body<T, KM, PROF>(b, g, a...);
    }
};

// The sizes the QR's panel kernels are launched with.  qr_plan (below: what qil_qr_plan hands to the tests) and the launchers
// read the same functions, so the plan cannot drift from what runs.  esz: bytes per element.
constexpr size_t QR_LDS_BUDGET = 150 * 1024;
inline size_t hh_panel_lds_bytes(size_t esz, long long m, int b) { return (size_t)((m + 1) | 1) * b * esz + 2048; }
inline bool hh_panel_fits_sized(size_t esz, long long m, int b) {
    return b <= 32 && m <= 64 * 19 && hh_panel_lds_bytes(esz, m, b) <= QR_LDS_BUDGET;
}
// the rows-per-lane variant hh_panel_launch instantiates for m rows
inline int hh_panel_km(long long m) {
    const int km = (int)((m + 63) / 64);
    return km <= 2 ? 2 : km <= 4 ? 4 : km <= 6 ? 6 : km <= 8 ? 8 : km <= 9 ? 9 : km <= 13 ? 13 : 19;
}
template <class T>
int hh_panel_waves_of(int km) {
    switch (km) {
        case 2: return hh_panel_waves<T, 2>();
        case 4: return hh_panel_waves<T, 4>();
        case 6: return hh_panel_waves<T, 6>();
        case 8: return hh_panel_waves<T, 8>();
        case 9: return hh_panel_waves<T, 9>();
        case 13: return hh_panel_waves<T, 13>();
        default: return hh_panel_waves<T, 19>();
    }
}
// LDS of the CGS2 kernel with its rows x n slice staged (gs_fused_k<T, true>)
inline size_t gs_fused_lds_bytes(size_t esz, long long rows, long long n) {
    return ((size_t)2 * (n + (n & 1)) + (size_t)(rows | 1) * n) * esz;
}
// rows per chunk of the tall-skinny tree
inline long long tsqr_chunk_rows(long long m) { return std::max<long long>(512, (m / 512 + 255) / 256 * 256); }

// true when the panel fits (LDS and rows-per-lane budget); launches it
template <class T>
bool hh_panel_fits(long long m, int b) {
    return hh_panel_fits_sized(sizeof(T), m, b);
}
template <class T>
int hh_panel_launch(qil_context* ctx, T* P, long long lda, long long m, int b, T* R, long long ldr, const double* ref_norm) {
    const size_t lds = hh_panel_lds_bytes(sizeof(T), m, b);
#define QIL_HHP(KMv)                                                                                                   \
    case KMv:                                                                                                          \
        QIL_TRY((qil_klaunch<hh_panel_k<T, KMv>>(ctx, dim3(1), dim3(64 * hh_panel_waves<T, KMv>()), lds, P, lda, (int)m, b, R, \
                           ldr, ref_norm, (long long*)nullptr)));                                                                             \
        break
    switch (hh_panel_km(m)) {
        QIL_HHP(2);
        QIL_HHP(4);
        QIL_HHP(6);
        QIL_HHP(8);
        QIL_HHP(9);
        QIL_HHP(13);
        QIL_HHP(19);
    }
#undef QIL_HHP
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

// launches gs_fused with the slice in LDS whenever rows_per_workgroup x n fits
template <class T>
int gs_fused_launch(qil_context* ctx, unsigned nwg, T* A, long long lda, long long mtot, int n, T* R, long long ldr,
                    const double* ref_norm, long long chunk_rows) {
    const long long rows = chunk_rows > 0 ? std::min(chunk_rows, mtot) : mtot;
    const size_t lds = gs_fused_lds_bytes(sizeof(T), rows, n);
    if (lds <= QR_LDS_BUDGET) {
        QIL_TRY((qil_klaunch<gs_fused_k<T, true>>(ctx, dim3(nwg), dim3(1024), lds, A, lda, mtot, n, R, ldr, ref_norm, chunk_rows)));
    } else {
        QIL_TRY((qil_klaunch<gs_fused_k<T, false>>(ctx, dim3(nwg), dim3(1024), (size_t)n * sizeof(T), A, lda, mtot, n, R, ldr, ref_norm, chunk_rows)));
    }
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

// Optional out-arguments of qr_impl: *orthonormal = the factorisation was CholeskyQR2 with its first-order second pass, so
// Q^H Q = I to O(|E|^2) < 1e-15 by construction (qr_reorthogonalise need not measure it).  rinv (with R): CholeskyQR2 also
// hands over R^-1 (n x n, ld n) in a block of its own for the certificate that follows (the caller frees it); other routes
// leave *rinv null.
template <class T>
int qr_impl(qil_context* ctx, long long m, long long n, T* A, long long lda, T* R, long long ldr, bool* orthonormal = nullptr,
            void** rinv = nullptr);
template <class T>
int gemm_dispatch(qil_context* ctx, int opA, int opB, long long m, long long n, long long k, const T* A,
                  long long lda, const T* B, long long ldb, T* C, long long ldc, const gemm_batch& batch);

// ------------------------------------------------------------------ block one-sided Jacobi (large column counts)
// The scalar tournament above moves the whole matrix through L2 once per ROUND (cols - 1 rounds per sweep,
// one rotation per column pair per round).  For hundreds to thousands of columns the same orthogonalisation
// is done on BLOCKS of BJ_B columns: a round pairs the blocks, and for every pair
//     G = P^H P        (P = the pair's 2 BJ_B columns)            batched MFMA GEMM, split over K
//     G = L L^H,  one-sided Jacobi on L^H  =>  J with J^H G J diagonal   (one workgroup, all in LDS)
//     [P; V_P] <- [P; V_P] J                                       batched MFMA GEMM
// so a sweep is (cols / BJ_B - 1) rounds of GEMM-shaped work.  The inner factorisation goes through the
// Cholesky factor, not G itself, so small singular directions inside a pair are still resolved relative to
// their own scale.  The update writes each block straight to the slot where the NEXT round's partner is
// adjacent (column-block scatter of the GEMM), so pairs are always 64 contiguous columns and nothing is
// ever copied just to re-pair.  The scalar tournament then runs as the convergence check / polish.
constexpr int BJ_B = 32;
constexpr int BJ_W = 2 * BJ_B;

// The visit's sweep is run as two-sided rotations on G itself (G <- R^H G R, angles from the current 2 x 2 blocks): no
// factorisation, no dot products, three short phases per round.  (The first version -- Cholesky G = L L^H followed by a
// one-sided sweep on L^H -- converged in the same number of block sweeps at ~1.7x the cost per visit and was removed.)
template <class T>
__device__ __forceinline__ void bj_pair_evd_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ Gm, T* __restrict__ Jm, double tol,
                                                    int max_sweeps, int* __restrict__ flag,
                                                    const int* __restrict__ big_second,
                                                    const double* __restrict__ negligible) {
    constexpr int N = BJ_W, LD = N + 1;
    extern __shared__ __attribute__((aligned(16))) char bj_smem[];
    T* Aw = reinterpret_cast<T*>(bj_smem);
    T* Vw = Aw + N * LD;
    __shared__ double d0[N], lam[N];
    __shared__ int s_any, dest[N];
    const int tid = threadIdx.x;
    const T* G = Gm + (long long)blockIdx.x * N * N;
    T* J = Jm + (long long)blockIdx.x * N * N;
    if (tid == 0) s_any = 0;
    for (int t = tid; t < N * N; t += 512) Aw[(t % N) + LD * (t / N)] = G[t];
    __syncthreads();
    if (tid < N) d0[tid] = reinterpret_cast<const double*>(&Aw[tid + LD * tid])[0];
    __syncthreads();
    int any = 0, work = 0;
    float worst = 0.f;
    const double ng = negligible ? *negligible : 0.0;
    for (int t = tid; t < N * N; t += 512) {
        const int r = t % N, c = t / N;
        if (r < c && !(d0[r] < ng || d0[c] < ng)) {
            const double g2 = abs2_t(Aw[r + LD * c]), dd = d0[r] * d0[c];
            if (g2 > tol * tol * dd) any = 1;                 // above the convergence threshold
            if (g2 > 1e-32 * dd) work = 1;                    // worth rotating at all
            if (dd > 0) worst = fmaxf(worst, (float)sqrt(g2 / dd));
        }
    }
    if (any) atomicOr(flag, 1);
    if (worst > 0.f) atomicMax(reinterpret_cast<unsigned*>(flag) + 1, __float_as_uint(worst));
    if (work) s_any = 1;
    __syncthreads();
    if (!s_any) {
        for (int t = tid; t < N * N; t += 512) {
            T v{};
            if (t % N == t / N) reinterpret_cast<double*>(&v)[0] = 1.0;
            J[t] = v;
        }
        return;
    }
    {
        __shared__ double rc[N / 2], rs[N / 2], rpr[N / 2], rpi[N / 2];
        __shared__ int rp[N / 2], rq[N / 2];
        for (int t = tid; t < N * N; t += 512) {
            const int r = t % N, c = t / N;
            T v{};
            if (r == c) reinterpret_cast<double*>(&v)[0] = 1.0;
            Vw[r + LD * c] = v;
        }
        __syncthreads();
        const int lane = tid & 15, grp = tid >> 4;       // 32 groups of 16 lanes, one column pair each
        for (int sweep = 0; sweep < max_sweeps; ++sweep) {
            for (int round = 0; round < N - 1; ++round) {
                // phase A: rotation of every pair from the current 2 x 2 blocks
                if (tid < N / 2) {
                    int p, q;
                    if (tid == 0) {
                        p = N - 1;
                        q = round;
                    } else {
                        p = (round + tid) % (N - 1);
                        q = (round + N - 1 - tid) % (N - 1);
                    }
                    if (p > q) {
                        const int t2 = p;
                        p = q;
                        q = t2;
                    }
                    const double al = reinterpret_cast<const double*>(&Aw[p + LD * p])[0];
                    const double be = reinterpret_cast<const double*>(&Aw[q + LD * q])[0];
                    const T g = Aw[p + LD * q];
                    const double gr = reinterpret_cast<const double*>(&g)[0];
                    const double gi = sizeof(T) == 16 ? reinterpret_cast<const double*>(&g)[1] : 0.0;
                    double c = 1.0, sn = 0.0, pr = 1.0, pi = 0.0;
                    bool big;
                    if (al < ng || be < ng || !jacobi_rotation<sizeof(T) == 16>(al, be, gr, gi, 1e-15, c, sn, pr, pi, big)) {
                        c = 1.0;
                        sn = 0.0;
                    }
                    rp[tid] = p;
                    rq[tid] = q;
                    rc[tid] = c;
                    rs[tid] = sn;
                    rpr[tid] = pr;
                    rpi[tid] = pi;
                }
                __syncthreads();
                {   // phase B: columns p, q of G and of J (all of a lane's loads first: a rolled loop pays one LDS
                    // latency per trip)
                    const int p = rp[grp], q = rq[grp];
                    const double c = rc[grp], sn = rs[grp], pr = rpr[grp], pi = rpi[grp];
                    if (sn != 0.0) {
                        constexpr int NR = N / 16;
                        T x[NR], y[NR], u[NR], w[NR];
    #pragma unroll
                        for (int t = 0; t < NR; ++t) {
                            const int r = lane + 16 * t;
                            x[t] = Aw[r + LD * p];
                            y[t] = Aw[r + LD * q];
                            u[t] = Vw[r + LD * p];
                            w[t] = Vw[r + LD * q];
                        }
    #pragma unroll
                        for (int t = 0; t < NR; ++t) {
                            const int r = lane + 16 * t;
                            rotate_pair(x[t], y[t], c, sn, pr, pi);
                            rotate_pair(u[t], w[t], c, sn, pr, pi);
                            Aw[r + LD * p] = x[t];
                            Aw[r + LD * q] = y[t];
                            Vw[r + LD * p] = u[t];
                            Vw[r + LD * q] = w[t];
                        }
                    }
                }
                __syncthreads();
                {   // phase C: rows p, q of G (R^H from the left = the conjugate rotation)
                    const int p = rp[grp], q = rq[grp];
                    const double c = rc[grp], sn = rs[grp], pr = rpr[grp], pi = rpi[grp];
                    if (sn != 0.0) {
                        constexpr int NR = N / 16;
                        T x[NR], y[NR];
    #pragma unroll
                        for (int t = 0; t < NR; ++t) {
                            const int cc = lane + 16 * t;
                            x[t] = Aw[p + LD * cc];
                            y[t] = Aw[q + LD * cc];
                        }
    #pragma unroll
                        for (int t = 0; t < NR; ++t) {
                            const int cc = lane + 16 * t;
                            rotate_pair(x[t], y[t], c, sn, pr, -pi);
                            Aw[p + LD * cc] = x[t];
                            Aw[q + LD * cc] = y[t];
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (tid < N) lam[tid] = reinterpret_cast<const double*>(&Aw[tid + LD * tid])[0];
        __syncthreads();
    }
    // de Rijk ordering at block level: the rotated columns leave sorted by norm (= eigenvalue of G), the
    // larger half to the block with the smaller tournament label -- without it the sweeps count doubles
    if (tid < N) {
        int rank = 0;
        const double mine = lam[tid];
        for (int k = 0; k < N; ++k) rank += (lam[k] > mine || (lam[k] == mine && k < tid)) ? 1 : 0;
        dest[tid] = big_second[blockIdx.x] ? (rank + N / 2) % N : rank;
    }
    __syncthreads();
    // J is a product of a few thousand rotations: one Newton-Schulz step J (3 I - J^H J) / 2 brings it back to
    // unitary at rounding level, otherwise the deviation accumulates over the hundreds of rounds V goes through
    for (int t = tid; t < N * N; t += 512) {
        const int r = t % N, c = t / N;
        T acc{};
        for (int k = 0; k < N; ++k) acc = fma_t(conj_t(Vw[k + LD * r]), Vw[k + LD * c], acc);
        acc = scale_t(acc, -0.5);
        if (r == c) reinterpret_cast<double*>(&acc)[0] += 1.5;
        Aw[r + LD * c] = acc;                                  // E = (3 I - J^H J) / 2
    }
    __syncthreads();
    for (int t = tid; t < N * N; t += 512) {
        const int r = t % N, c = t / N;
        T acc{};
        for (int k = 0; k < N; ++k) acc = fma_t(Vw[r + LD * k], Aw[k + LD * c], acc);
        J[r + N * dest[c]] = acc;
    }
}
template <class T>
struct bj_pair_evd_k {
    static constexpr int NT = 512, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        bj_pair_evd_body<T>(b, g, a...);
    }
};

// Runs block sweeps on [Wk; I] (copied into a padded, double-buffered work area) until no pair's Gram matrix
// has a relative off-diagonal above `tol` (or `max_sweeps`).  Returns the buffer holding the result:
// rows [0, rows) = rotated Wk, rows [rows, rows + cols) = accumulated V, `cols_pad` columns in tournament
// order (padding columns are entirely zero).
template <class T>
int block_jacobi(qil_context* ctx, long long rows, long long cols, const T* Wk, long long ldw, double tol,
                 int max_sweeps, void** xbuf, long long* ldx_out, long long* cols_pad_out, bool* converged,
                 const double* negligible) {
    *converged = false;
    const long long cpad = (cols + BJ_W - 1) / BJ_W * BJ_W;
    const int nb = (int)(cpad / BJ_B), np = nb / 2;
    const long long rt = rows + cols, ldx = rt;
    void *xa = nullptr, *xb = nullptr, *gbuf = nullptr, *jbuf = nullptr, *flag = nullptr, *cmapd = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(ldx * cpad) * sizeof(T), &xa));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(ldx * cpad) * sizeof(T), &xb));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)np * BJ_W * BJ_W * sizeof(T), &gbuf));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)np * BJ_W * BJ_W * sizeof(T), &jbuf));
    QIL_TRY(qil_ctx_alloc(ctx, 256, &flag));
    // tournament bookkeeping: lab[r][s] = block label in slot s during round r (pairs = slots 2i, 2i+1);
    // cmap[r][s] = slot of that label in round r + 1
    const int nr = std::max(nb - 1, 1);
    std::vector<int> lab((size_t)nr * nb), pos((size_t)nr * nb), cmap((size_t)nr * nb + (size_t)nr * np);
    for (int r = 0; r < nr; ++r)
        for (int i = 0; i < np; ++i) {
            int p, q;
            if (i == 0) {
                p = nb - 1;
                q = r;
            } else {
                p = (r + i) % (nb - 1);
                q = (r + nb - 1 - i) % (nb - 1);
            }
            if (nb == 2) { p = 1; q = 0; }
            lab[(size_t)r * nb + 2 * i] = p;
            lab[(size_t)r * nb + 2 * i + 1] = q;
            pos[(size_t)r * nb + p] = 2 * i;
            pos[(size_t)r * nb + q] = 2 * i + 1;
        }
    for (int r = 0; r < nr; ++r)
        for (int s2 = 0; s2 < nb; ++s2)
            cmap[(size_t)r * nb + s2] = pos[(size_t)((r + 1) % nr) * nb + lab[(size_t)r * nb + s2]];
    int* big2 = cmap.data() + (size_t)nr * nb;      // [r][i]: 1 if the pair's SECOND slot holds the smaller label
    for (int r = 0; r < nr; ++r)
        for (int i = 0; i < np; ++i)
            big2[(size_t)r * np + i] = lab[(size_t)r * nb + 2 * i] > lab[(size_t)r * nb + 2 * i + 1] ? 1 : 0;
    QIL_TRY(qil_ctx_alloc(ctx, cmap.size() * sizeof(int), &cmapd));
    QIL_HIP(hipMemcpyAsync(cmapd, cmap.data(), cmap.size() * sizeof(int), hipMemcpyHostToDevice, qil_stream(ctx)));
    T* Xc = static_cast<T*>(xa);
    T* Xn = static_cast<T*>(xb);
    QIL_TRY(qil_dev_zero(ctx, Xc, (size_t)(ldx * cpad) * sizeof(T)));
    QIL_TRY(qil_dev_copy2d(ctx, Xc, (size_t)ldx * sizeof(T), Wk, (size_t)ldw * sizeof(T), (size_t)rows * sizeof(T),
                             (size_t)cols));
    QIL_TRY((qil_klaunch<set_identity_k<T>>(ctx, dim3((unsigned)std::min<long long>((cols * cols + 255) / 256, 65536)), dim3(256), 0, Xc + rows, ldx, (int)cols)));
    const size_t lds = (size_t)2 * BJ_W * (BJ_W + 1) * sizeof(T);
    const int opH = sizeof(T) == 16 ? 2 : 1;
    static const int inner_sweeps = 1;
    gemm_batch bg, bu;
    bg.count = np;
    bg.a_bs = bg.b_bs = (long long)BJ_W * ldx;
    bg.c_bs = BJ_W * BJ_W;
    bu.count = np;
    bu.a_bs = (long long)BJ_W * ldx;
    bu.b_bs = BJ_W * BJ_W;
    bu.cmap_blk = BJ_B;
    int status = QIL_OK;
    for (int sweep = 0; sweep < max_sweeps && status == QIL_OK; ++sweep) {
        QIL_TRY(qil_dev_zero(ctx, flag, 2 * sizeof(int)));
        for (int r = 0; r < nr && status == QIL_OK; ++r) {
            status = gemm_dispatch<T>(ctx, opH, 0, BJ_W, BJ_W, rows, Xc, ldx, Xc, ldx, static_cast<T*>(gbuf), BJ_W, bg);
            if (status != QIL_OK) break;
            QIL_TRY((qil_klaunch<bj_pair_evd_k<T>>(ctx, dim3((unsigned)np), dim3(512), lds, (const T*)gbuf, static_cast<T*>(jbuf), tol, inner_sweeps, (int*)flag, static_cast<const int*>(cmapd) + (size_t)nr * nb + (size_t)r * np, negligible)));
            bu.cmap = static_cast<const int*>(cmapd) + (size_t)r * nb;
            status = gemm_dispatch<T>(ctx, 0, 0, rt, BJ_W, BJ_W, Xc, ldx, static_cast<const T*>(jbuf), BJ_W, Xn, ldx, bu);
            std::swap(Xc, Xn);
        }
        int hh[2] = {0, 0};
        QIL_TRY(qil_read_back(ctx, hh, flag, 2 * sizeof(int)));
        float worst;
        memcpy(&worst, &hh[1], sizeof(float));
        if (getenv("QIL_SVD_DEBUG"))
            fprintf(stderr, "[svd] block sweep %d (cols %lld): above tol=%d, worst relative off-diagonal %.3g\n", sweep,
                    cols, hh[0], (double)worst);
        if (!hh[0]) {
            *converged = true;
            break;
        }
    }
    QIL_HIP(qil_stream_sync(ctx));   // cmap (host vector) upload has completed
    qil_ctx_free(ctx, Xc == xa ? xb : xa);
    qil_ctx_free(ctx, gbuf);
    qil_ctx_free(ctx, jbuf);
    qil_ctx_free(ctx, flag);
    qil_ctx_free(ctx, cmapd);
    *xbuf = Xc;
    *ldx_out = ldx;
    *cols_pad_out = cpad;
    return status;
}

// out[0] = rel * sum_j norms[j]^2  (the threshold below which a column counts as rounding residue)
__device__ __forceinline__ void negligible_threshold_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ norms, int n, double rel,
                                                            double* __restrict__ out) {
    __shared__ double red[4];
    double v = 0;
    for (int j = threadIdx.x; j < n; j += 256) v = fma(norms[j], norms[j], v);
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = rel * ((red[0] + red[1]) + (red[2] + red[3]));
}
struct negligible_threshold_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        negligible_threshold_body(b, g, a...);
    }
};

// out[0] = max over i != j of |G[i, j]| (as the bit pattern of a non-negative double: atomicMax on the integer view)
template <class T>
__device__ __forceinline__ void offdiag_max_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ G, long long ldg, long long n,
                                                   unsigned long long* __restrict__ out) {
    double v = 0;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < n * n; t += (long long)gridDim.x * 256) {
        const long long i = t % n, j = t / n;
        if (i != j) v = fmax(v, sqrt(abs2_t(G[i + ldg * j])));
    }
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if ((int)threadIdx.x < s2) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s2]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__double_as_longlong(red[0]));
}
template <class T>
struct offdiag_max_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        offdiag_max_body<T>(b, g, a...);
    }
};

// CGS2 keeps Q orthonormal only while the operand is numerically of full rank ("twice is enough" needs
// kappa * eps < 1).  Operands that are not -- product bonds before their truncation, sketches wider than the rank,
// spectra graded down to 1e-14 -- leave late columns whose residual is rounding noise with O(1) overlaps, and the
// singular values of R are then not those of the operand.  Q^H Q is measured (one small GEMM + a max-reduction), and
// while it is not the identity to 1e-11, Q is factored once more: Q = Q2 R2 is a well-conditioned problem (columns
// lying in the span of earlier ones come out as zero columns), and R <- R2 R.  At most two extra factorisations.
// known_orthonormal: what qr_impl reported for Q.  rinv (may be null): an R^-1 the caller holds; a re-factorisation frees it.
template <class T>
int qr_reorthogonalise(qil_context* ctx, long long m, long long n, T* Q, long long ldq, T* R, long long ldr, bool known_orthonormal,
                       void** rinv, bool dbg, bool* orthonormal = nullptr) {
    if (orthonormal) *orthonormal = true;
    if (n < 2) return QIL_OK;
    // r06: nothing to measure after a CholeskyQR2 whose second pass was the first-order one (A/B with the check forced on,
    // profiles/r06_qr_recheck_ab.txt: bit-identical results, zT compression 64.2 -> 62.6 ms, compress! chi 256 45.2 -> 44.4 ms)
    qil_qr_report* const rep = ctx->qr_report;               // null outside qil_qr_host
    if (known_orthonormal) {
        if (rep) rep->skipped_check = 1;
        return QIL_OK;
    }
    void *gbuf = nullptr, *mx = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(n * n) * sizeof(T), &gbuf));
    QIL_TRY(qil_ctx_alloc(ctx, 256, &mx));
    for (int pass = 0; pass < 3; ++pass) {
        QIL_TRY(qil_dev_zero(ctx, mx, sizeof(unsigned long long)));
        QIL_TRY(gemm_dispatch<T>(ctx, sizeof(T) == 16 ? 2 : 1, 0, n, n, m, Q, ldq, Q, ldq, static_cast<T*>(gbuf), n));
        QIL_TRY((qil_klaunch<offdiag_max_k<T>>(ctx, dim3((unsigned)std::min<long long>((n * n + 255) / 256, 1024)), dim3(256), 0, (const T*)gbuf, n, n, (unsigned long long*)mx)));
        double worst = 0;
        QIL_TRY(qil_read_back(ctx, &worst, mx, sizeof(double)));
        if (dbg) fprintf(stderr, "[qr] max |Q^H Q - I| off-diagonal %.3g\n", worst);
        if (orthonormal) *orthonormal = !(worst > 1e-9);
        if (rep) rep->worst[pass] = worst, rep->passes = pass + 1;
        if (!(worst > 1e-11) || pass == 2) break;
        if (rep) ++rep->repairs;
        ctx->qr_report = nullptr;                            // the report describes the outer factorisation
        const int st2 = qr_impl<T>(ctx, m, n, Q, ldq, static_cast<T*>(gbuf), n);           // Q <- Q2, gbuf = R2
        ctx->qr_report = rep;
        QIL_TRY(st2);
        if (R) {
            if (rinv && *rinv) {                                 // R changes: an inverse kept for the certificate is stale
                qil_ctx_free(ctx, *rinv);
                *rinv = nullptr;
            }
            void* rnew = nullptr;
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(n * n) * sizeof(T), &rnew));
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, n, n, n, static_cast<const T*>(gbuf), n, (const T*)R, ldr,
                                     static_cast<T*>(rnew), n));
            QIL_TRY(qil_dev_copy2d(ctx, R, (size_t)ldr * sizeof(T), rnew, (size_t)n * sizeof(T), (size_t)n * sizeof(T),
                                     (size_t)n));
            qil_ctx_free(ctx, rnew);
        }
    }
    qil_ctx_free(ctx, gbuf);
    qil_ctx_free(ctx, mx);
    return QIL_OK;
}

// ------------------------------------------------------------------ "nothing can be truncated" certificate
// A gauge sweep that truncates with a cutoff (canonicalize!(cutoff = 1e-12), the first pass of compress!) pays a full SVD
// per site even where no singular value can go: the rule drops a tail only while sum(sigma_dropped^2) <= cutoff sum(sigma^2),
// so nothing is dropped whenever sigma_min^2 > cutoff |A|_F^2.  With the triangular factor R of the site's thin QR at hand,
// sigma_min(R) >= 1 / |R^-1|_2 >= 1 / |R^-1|_F, and R^-1 is a blocked triangular inversion (64 x 64 diagonal blocks by back
// substitution, the rest MFMA GEMMs): a rigorous bound for the price of a few small launches.  Where it holds, the thin QR
// IS the gauge step (the kept space is the whole space; Q differs from the SVD's U by a unitary on the bond, which no
// gauge-invariant quantity sees) and the Jacobi iteration is skipped.  Rank-deficient operands -- every product bond of
// the signal pipelines -- fail the first test (sigma_min <= min |r_ii|) before anything is inverted.
template <class T>
__device__ __forceinline__ void tri_stats_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ R, long long ldr, int k, int upper_only,
                                                 double* __restrict__ out /* per block: [fro2, min |r_ii|^2] */) {
    __shared__ double red[8];
    double f = 0, d = 1e300;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < (long long)k * k; t += 256LL * gridDim.x) {
        const int i = (int)(t % k), j = (int)(t / k);
        if (upper_only && i > j) continue;
        const double a = abs2_t(R[i + ldr * j]);
        f += a;
        if (i == j) d = fmin(d, a);
    }
    f = wave_sum(f);
    for (int off = 32; off; off >>= 1) d = fmin(d, __shfl_xor(d, off));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave] = f;
        red[4 + wave] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        out[2 * blockIdx.x + 1] = fmin(fmin(red[4], red[5]), fmin(red[6], red[7]));
    }
}
template <class T>
struct tri_stats_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        tri_stats_body<T>(b, g, a...);
    }
};

__device__ __forceinline__ double inv_t(double u) { return 1.0 / u; }
__device__ __forceinline__ c64 inv_t(c64 u) {
    const double s = 1.0 / (u.re * u.re + u.im * u.im);
    return c64{u.re * s, -u.im * s};
}
__device__ __forceinline__ double mul_t(double a, double b) { return a * b; }
__device__ __forceinline__ c64 mul_t(c64 a, c64 b) { return c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ double neg_t(double a) { return -a; }
__device__ __forceinline__ c64 neg_t(c64 a) { return c64{-a.re, -a.im}; }

// X (column block b of the k x k result) = inverse of the 64 x 64 (or smaller, last) upper-triangular diagonal block b of R:
// thread j solves U x_j = e_j by back substitution, the block in LDS
template <class T>
__device__ __forceinline__ void trtri_diag_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ R, long long ldr, int k, T* __restrict__ X, long long ldx) {
    extern __shared__ __attribute__((aligned(16))) char trtri_smem[];
    T* U = reinterpret_cast<T*>(trtri_smem);
    T* Xs = U + 64 * 65;
    const int b0 = blockIdx.x * 64, nb = min(64, k - b0), j = threadIdx.x;
    for (int c = 0; c < nb; ++c)
        if (j < nb) U[j + 65 * c] = (j <= c) ? R[(b0 + j) + ldr * (long long)(b0 + c)] : T{};
    __syncthreads();
    if (j < nb) {
        // x_jj = 1 / u_jj; x_ij = -(sum_{l = i + 1 .. j} u_il x_lj) / u_ii; the solved entries of column j stay in LDS
        T* x = Xs + 65 * j;
        x[j] = inv_t(U[j + 65 * j]);
        for (int i = j - 1; i >= 0; --i) {
            T acc{};
            for (int l = i + 1; l <= j; ++l) acc = fma_t(U[i + 65 * l], x[l], acc);
            x[i] = neg_t(mul_t(acc, inv_t(U[i + 65 * i])));
        }
    }
    __syncthreads();
    for (int c = 0; c < nb; ++c)
        if (j < nb && j <= c) X[(b0 + j) + ldx * (long long)(b0 + c)] = Xs[j + 65 * c];
}
template <class T>
struct trtri_diag_k {
    static constexpr int NT = 64, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        trtri_diag_body<T>(b, g, a...);
    }
};

// The off-diagonal blocks of Xinv = R^-1 (k x k, ld k) from its inverted diagonal blocks of width `blk` (already in place):
// neighbouring blocks are merged level by level, [A B; 0 C]^-1 = [A^-1, -A^-1 B C^-1; 0, C^-1]  (MFMA GEMMs)
template <class T>
int trtri_merge(qil_context* ctx, const T* R, long long ldr, int k, T* Xinv, int blk) {
    const int nb = (k + blk - 1) / blk;
    struct Blk { int start, size; };
    std::vector<Blk> cur;
    for (int b = 0; b < nb; ++b) cur.push_back(Blk{b * blk, std::min(blk, k - b * blk)});
    if (cur.size() < 2) return QIL_OK;
    void* tmp = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)k * k * sizeof(T), &tmp));
    T* Tm = static_cast<T*>(tmp);
    // (the off-diagonal blocks of Xinv are zero on entry: X12 = 0 - A^-1 T needs no separate negation; the equal-sized merges of
    // a level go out as ONE strided batch per product)
    gemm_batch sub;
    sub.subtract = 1;
    while (cur.size() > 1) {
        std::vector<Blk> next;
        const size_t npairs = cur.size() / 2;
        size_t nuni = 0;
        const int sz = cur[0].size;
        while (nuni < npairs && cur[2 * nuni].size == sz && cur[2 * nuni + 1].size == sz) ++nuni;
        if (nuni < 2) nuni = 0;
        if (nuni) {
            const int a0 = cur[0].start, c0 = a0 + sz;
            gemm_batch b1, b2 = sub;
            b1.count = b2.count = (int)nuni;
            b1.a_bs = 2LL * sz * (1 + ldr);
            b1.b_bs = 2LL * sz * (1 + (long long)k);
            b1.c_bs = (long long)sz * sz;
            b2.a_bs = 2LL * sz * (1 + (long long)k);
            b2.b_bs = (long long)sz * sz;
            b2.c_bs = 2LL * sz * (1 + (long long)k);
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, sz, sz, sz, R + a0 + ldr * (long long)c0, ldr, Xinv + c0 + (long long)k * c0, k, Tm, sz, b1));
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, sz, sz, sz, Xinv + a0 + (long long)k * a0, k, Tm, sz, Xinv + a0 + (long long)k * c0, k, b2));
        }
        for (size_t i = 0; i + 1 < cur.size(); i += 2) {
            const int a0 = cur[i].start, sa = cur[i].size, c0 = cur[i + 1].start, sc = cur[i + 1].size;
            if (i / 2 >= nuni) {
                // T = B C^-1 (sa x sc), X12 = -(A^-1 T)
                QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, sa, sc, sc, R + a0 + ldr * (long long)c0, ldr, Xinv + c0 + (long long)k * c0, k, Tm, sa));
                QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, sa, sc, sa, Xinv + a0 + (long long)k * a0, k, Tm, sa, Xinv + a0 + (long long)k * c0, k, sub));
            }
            next.push_back(Blk{a0, sa + sc});
        }
        if (cur.size() & 1) next.push_back(cur.back());
        cur.swap(next);
    }
    QIL_HIP(hipGetLastError());
    qil_ctx_free(ctx, tmp);
    return QIL_OK;
}

// Xinv (k x k, ld k, zero below the diagonal) = R^-1 for upper-triangular R
template <class T>
int trtri_upper(qil_context* ctx, const T* R, long long ldr, int k, T* Xinv) {
    QIL_TRY(qil_dev_zero(ctx, Xinv, (size_t)k * k * sizeof(T)));
    const int nb = (k + 63) / 64;
    constexpr size_t diag_lds = (size_t)2 * 64 * 65 * sizeof(T);
    QIL_TRY((qil_klaunch<trtri_diag_k<T>>(ctx, dim3((unsigned)nb), dim3(64), diag_lds, R, ldr, k, Xinv, (long long)k)));
    QIL_HIP(hipGetLastError());
    return trtri_merge<T>(ctx, R, ldr, k, Xinv, 64);
}

// ------------------------------------------------------------------ Cholesky QR (CholeskyQR2) for the gauge sweeps
// A thin QR of a well-conditioned operand needs no column-by-column chain: G = A^H A (one MFMA GEMM), G = R^H R, Q = A R^-1,
// and once more on Q (CholeskyQR2: orthonormal to rounding while kappa(A)^2 eps << 1).  The gauge sweeps of compress! /
// canonicalize! factor sites whose conditioning the truncation certificate bounds anyway (it declines beyond kappa ~ 5e5),
// and a blocked Householder QR of 512 x 256 is ~80 small launches with eight 50-70 us one-workgroup panels in them.
// chol_inv_block16: R and R^-1 of a Hermitian positive definite diagonal block of up to 64 columns in ONE workgroup, with the
// column chain cut to 16 columns at a time.  (The first version -- a register-tiled elimination of the whole block on 32 x 32
// threads, one workgroup barrier and an LDS round trip per COLUMN: 64 x ~1300 cycles = 35 us per block, the largest single item
// of a CholeskyQR2 gauge step -- was removed; this one takes 19 us, tools/micro/chol_block_cost.hip.)  The block lives in LDS
// as a full Hermitian 64 x 64 array and is factored by 16-column sub-blocks:
//   D(b)  ONE wave eliminates the 16 x 16 diagonal sub-block of [S | I] in registers (lane (i, g) = four columns of row i):
//         a step is one reciprocal, the multipliers and the pivot row passed lane to lane (chol16_step) and 8 FMAs -- no
//         barrier, no LDS; R_bb = D^-1/2 U and X_bb = R_bb^-1 = E^H D^-1/2 go back to LDS;
//   P(b)  R(b, c) = X_bb^H S(b, c), c > b                (one 16 x 16 x 16 matrix-core tile per wave)
//   T(b)  S(c, d) -= R(b, c)^H R(b, d), b < c <= d       (matrix-core tiles over the four waves)
// and R^-1's off-diagonal sub-blocks by two levels of [A B; 0 C]^-1 = [A^-1, -A^-1 B C^-1; 0, C^-1] merges on the matrix
// cores.  12 barriers + 64 short register steps instead of 64 barrier-separated column steps.
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
typedef unsigned qil_v2u __attribute__((ext_vector_type(2)));
// lane J of every 16-lane row to all lanes of that row (DPP row_newbcast: a plain VALU move, no scalar-register round trip)
template <int J>
__device__ __forceinline__ double row_bcast_f64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x150 + J, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x150 + J, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// row GS of the wave (lanes 16 GS .. 16 GS + 15) to all four rows, lane by lane (gfx950 v_permlane32_swap + v_permlane16_swap:
// swap(v, v) of the first returns [r0 r1 r0 r1] / [r2 r3 r2 r3], of the second [w0 w0 w2 w2] / [w1 w1 w3 w3];
// tools/micro/permlane_probe.hip prints both)
template <int GS>
__device__ __forceinline__ unsigned rowgroup_bcast_u32(unsigned v) {
    const qil_v2u a = __builtin_amdgcn_permlane32_swap(v, v, true, false);
    const unsigned w = a[GS >> 1];
    const qil_v2u b = __builtin_amdgcn_permlane16_swap(w, w, true, false);
    return b[GS & 1];
}
template <int GS>
__device__ __forceinline__ double rowgroup_bcast_f64(double v) {
    const unsigned lo = rowgroup_bcast_u32<GS>((unsigned)__double2loint(v)), hi = rowgroup_bcast_u32<GS>((unsigned)__double2hiint(v));
    return __hiloint2double((int)hi, (int)lo);
}
// One column step of the 16 x 16 elimination of [S | I] held by ONE wave: lane (i = lane & 15, g = lane >> 4) keeps columns
// 4 g .. 4 g + 3 of row i of S and of E.  Pivot d_J through a scalar register, the multipliers m_i = S(i, J) / d_J from row
// group J / 4 to all four, the pivot row within each row group by DPP; 8 FMAs per lane (complex: 32).
template <bool CX, int J, int B>
__device__ __forceinline__ void chol16_elem(double (&sr)[4], double (&si)[4], double (&er)[4], double (&ei)[4], double mr, double mi) {
    if constexpr (12 + B > J) {                                      // some row group still has column 4 g + B > J
        const double pr = row_bcast_f64<J>(sr[B]);
        if constexpr (CX) {
            const double pi = row_bcast_f64<J>(si[B]);
            sr[B] = fma(mi, pi, fma(-mr, pr, sr[B]));
            si[B] = fma(-mi, pr, fma(-mr, pi, si[B]));
        } else {
            sr[B] = fma(-mr, pr, sr[B]);
        }
    }
    if constexpr (B <= J) {                                          // E(J, k) = 0 beyond k = J
        const double pr = row_bcast_f64<J>(er[B]);
        if constexpr (CX) {
            const double pi = row_bcast_f64<J>(ei[B]);
            er[B] = fma(mi, pi, fma(-mr, pr, er[B]));
            ei[B] = fma(-mi, pr, fma(-mr, pi, ei[B]));
        } else {
            er[B] = fma(-mr, pr, er[B]);
        }
    }
}
template <bool CX, int J>
__device__ __forceinline__ void chol16_step(double (&sr)[4], double (&si)[4], double (&er)[4], double (&ei)[4], int li, double d0l,
                                            double piv_rel, double& dgl, double& worst) {
    constexpr int GJ = J >> 2, BJ = J & 3;
    asm volatile("" : "+v"(li));                                     // (keeps the 32 lane masks of the 16 steps from being hoisted: scalar-register spills)
    const double d = readlane_f64(sr[BJ], J + 16 * GJ);
    const double margin = fma(-piv_rel, readlane_f64(d0l, J), d);   // the pivot must stay above piv_rel times its original diagonal entry
    worst = fmin(worst, margin);
    const bool dead = !(margin > 0.0);
    const double inv = dead ? 0.0 : rcp_refined(d);
    const double mcr = rowgroup_bcast_f64<GJ>(sr[BJ]);
    double mci = 0.0;
    if constexpr (CX) mci = rowgroup_bcast_f64<GJ>(si[BJ]);
    const double sel = li > J ? inv : 0.0;
    if (li == J) dgl = dead ? 1.0 : d;
    const double mr = mcr * sel, mi = mci * sel;
    chol16_elem<CX, J, 0>(sr, si, er, ei, mr, mi);
    chol16_elem<CX, J, 1>(sr, si, er, ei, mr, mi);
    chol16_elem<CX, J, 2>(sr, si, er, ei, mr, mi);
    chol16_elem<CX, J, 3>(sr, si, er, ei, mr, mi);
}
template <bool CX, int... J>
__device__ __forceinline__ void chol16_steps(double (&sr)[4], double (&si)[4], double (&er)[4], double (&ei)[4], int li, double d0l,
                                             double piv_rel, double& dgl, double& worst, std::integer_sequence<int, J...>) {
    (chol16_step<CX, J>(sr, si, er, ei, li, d0l, piv_rel, dgl, worst), ...);
}
template <class T>
constexpr size_t chol16_lds() {
    return (size_t)(sizeof(T) / 8) * (2 * 64 * 65 + 32 * 33) * sizeof(double);
}
template <class T>
__device__ __forceinline__ void chol_inv_block16_body(const uint3, const uint3, const T* __restrict__ G, long long ldg, int nb,
                                                      T* __restrict__ Rout, long long ldr, T* __restrict__ Xout, long long ldx,
                                                      double piv_rel, int* __restrict__ flag) {
    constexpr bool CX = sizeof(T) == 16;
    constexpr int NP = CX ? 2 : 1;
    constexpr int N = 64, LD = 65, PL = N * LD, LT = 33, PT = 32 * LT;
    extern __shared__ __attribute__((aligned(16))) char c16_smem[];
    double* S = reinterpret_cast<double*>(c16_smem);                 // [NP][PL]: S, then R in its upper sub-blocks
    double* Si = S + (CX ? PL : 0);
    double* X = S + NP * PL;                                         // [NP][PL]: R^-1
    double* Xi = X + (CX ? PL : 0);
    double* Tm = X + NP * PL;                                        // [NP][PT]: the merges' B C^-1
    double* Ti = Tm + (CX ? PT : 0);
    __shared__ double d0[N];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nb16 = (nb + 15) >> 4;
    if (tid == 0) s_bad = 0;
    // ---- the block as a full Hermitian array (rows / columns beyond nb: identity), X = 0
    for (int t = tid; t < N * N; t += 256) {
        const int i = t & 63, k = t >> 6;
        X[i * LD + k] = 0.0;
        if constexpr (CX) Xi[i * LD + k] = 0.0;
        if (i > k) continue;
        double vr = (i == k) ? 1.0 : 0.0, vi = 0.0;
        if (k < nb) {
            const double* g = reinterpret_cast<const double*>(G + i + ldg * k);
            vr = g[0];
            if (CX && i != k) vi = g[1];
        }
        S[i * LD + k] = vr;
        S[k * LD + i] = vr;
        if constexpr (CX) {
            Si[i * LD + k] = vi;
            Si[k * LD + i] = -vi;
        }
        if (i == k) d0[i] = vr;
    }
    __syncthreads();
    for (int b = 0; b < nb16; ++b) {
        const int r0 = 16 * b;
        // ---- D(b)
        if (wave == 0) {
            double sr[4], si[4], er[4], ei[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * lk + q;
                sr[q] = S[(r0 + li) * LD + r0 + k];
                si[q] = CX ? Si[(r0 + li) * LD + r0 + k] : 0.0;
                er[q] = (k == li) ? 1.0 : 0.0;
                ei[q] = 0.0;
            }
            const double d0l = d0[r0 + li];
            double dgl = 1.0;
            double worst = 1.0;
            chol16_steps<CX>(sr, si, er, ei, li, d0l, piv_rel, dgl, worst, std::make_integer_sequence<int, 16>{});
            if (!(worst > 0.0) && lane == 0) s_bad = 1;
            const double rs = rsqrt(dgl), sq = sqrt(dgl);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // R(i, k) = U(i, k) / sqrt(d_i) (k > i), sqrt(d_i) on the diagonal;  X(k, i) = conj(E(i, k)) / sqrt(d_i) (k <= i)
                const int k = 4 * lk + q;
                S[(r0 + li) * LD + r0 + k] = k > li ? sr[q] * rs : (k == li ? sq : 0.0);
                if constexpr (CX) Si[(r0 + li) * LD + r0 + k] = k > li ? si[q] * rs : 0.0;
                X[(r0 + k) * LD + r0 + li] = k <= li ? er[q] * rs : 0.0;
                if constexpr (CX) Xi[(r0 + k) * LD + r0 + li] = k <= li ? -ei[q] * rs : 0.0;
            }
        }
        __syncthreads();
        if (b + 1 >= nb16) break;
        // ---- P(b): R(b, c) = X_bb^H S(b, c); wave -> c = b + 1 + wave.  out(p, q): first operand [p = li][k = lk], second [k = lk][q = li]
        {
            const int c = b + 1 + wave;
            if (c < nb16) {
                d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int t = r0 + 4 * ks + lk;
                    const double ar = X[t * LD + r0 + li], br = S[t * LD + 16 * c + li];
                    rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, rr, 0, 0, 0);
                    if constexpr (CX) {
                        // conj(x) s = (xr sr + xi si) + i (xr si - xi sr)
                        const double ai = Xi[t * LD + r0 + li], bi = Si[t * LD + 16 * c + li];
                        rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, rr, 0, 0, 0);
                        ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ri, 0, 0, 0);
                        ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ii, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    S[(r0 + lk + 4 * r) * LD + 16 * c + li] = rr[r];
                    if constexpr (CX) Si[(r0 + lk + 4 * r) * LD + 16 * c + li] = ri[r] - ii[r];
                }
            }
        }
        __syncthreads();
        // ---- T(b): S(c, d) -= R(b, c)^H R(b, d), b < c <= d
        {
            int idx = 0;
            for (int c = b + 1; c < nb16; ++c)
                for (int d = c; d < nb16; ++d, ++idx) {
                    if ((idx & 3) != wave) continue;
                    d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int t = r0 + 4 * ks + lk;
                        const double ar = S[t * LD + 16 * c + li], br = S[t * LD + 16 * d + li];
                        rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, rr, 0, 0, 0);
                        if constexpr (CX) {
                            const double ai = Si[t * LD + 16 * c + li], bi = Si[t * LD + 16 * d + li];
                            rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, rr, 0, 0, 0);
                            ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ri, 0, 0, 0);
                            ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ii, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        S[(16 * c + lk + 4 * r) * LD + 16 * d + li] -= rr[r];
                        if constexpr (CX) Si[(16 * c + lk + 4 * r) * LD + 16 * d + li] -= ri[r] - ii[r];
                    }
                }
        }
        __syncthreads();
    }
    // ---- R^-1: merges of neighbouring sub-blocks, then of the two halves.  X(A, C) = -X(A, A) [R(A, C) X(C, C)]
    for (int lvl = 0; lvl < 2; ++lvl) {
        const int sz = lvl == 0 ? 16 : 32;
        const int nmerge = lvl == 0 ? 2 : 1;
        // this wave's tile: level 0: merge = wave (one tile); level 1: tile (wave >> 1, wave & 1) of the one merge
        const int mg = lvl == 0 ? wave : 0, ti = lvl == 0 ? 0 : (wave >> 1), tj = lvl == 0 ? 0 : (wave & 1);
        const int a0 = 2 * sz * mg, c0 = a0 + sz;
        const bool act = mg < nmerge && c0 + 16 * tj < 16 * nb16;
        if (16 * nb16 <= sz) break;
        if (act) {
            d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
            for (int ks = 0; ks < sz / 4; ++ks) {
                const int t = c0 + 4 * ks + lk;
                const double ar = S[(a0 + 16 * ti + li) * LD + t], br = X[t * LD + c0 + 16 * tj + li];
                rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, rr, 0, 0, 0);
                if constexpr (CX) {
                    const double ai = Si[(a0 + 16 * ti + li) * LD + t], bi = Xi[t * LD + c0 + 16 * tj + li];
                    ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, ii, 0, 0, 0);
                    ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ri, 0, 0, 0);
                    ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ri, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Tm[(16 * (lvl == 0 ? mg : ti) + lk + 4 * r) * LT + 16 * tj + li] = CX ? rr[r] - ii[r] : rr[r];
                if constexpr (CX) Ti[(16 * (lvl == 0 ? mg : ti) + lk + 4 * r) * LT + 16 * tj + li] = ri[r];
            }
        }
        __syncthreads();
        if (act) {
            d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
            for (int ks = 0; ks < sz / 4; ++ks) {
                const int t = 4 * ks + lk;
                const double ar = X[(a0 + 16 * ti + li) * LD + a0 + t];
                const double br = Tm[(16 * (lvl == 0 ? mg : 0) + t) * LT + 16 * tj + li];
                rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, rr, 0, 0, 0);
                if constexpr (CX) {
                    const double ai = Xi[(a0 + 16 * ti + li) * LD + a0 + t];
                    const double bi = Ti[(16 * (lvl == 0 ? mg : 0) + t) * LT + 16 * tj + li];
                    ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, ii, 0, 0, 0);
                    ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ri, 0, 0, 0);
                    ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ri, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                X[(a0 + 16 * ti + lk + 4 * r) * LD + c0 + 16 * tj + li] = CX ? ii[r] - rr[r] : -rr[r];
                if constexpr (CX) Xi[(a0 + 16 * ti + lk + 4 * r) * LD + c0 + 16 * tj + li] = -ri[r];
            }
        }
        __syncthreads();
    }
    if (tid == 0 && s_bad) atomicOr(flag, 1);
    for (int t = tid; t < N * N; t += 256) {
        const int i = t & 63, k = t >> 6;
        if (i >= nb || k >= nb) continue;
        T rv{}, xv{};
        if (i <= k) {
            reinterpret_cast<double*>(&rv)[0] = S[i * LD + k];
            reinterpret_cast<double*>(&xv)[0] = X[i * LD + k];
            if constexpr (CX) {
                reinterpret_cast<double*>(&rv)[1] = Si[i * LD + k];
                reinterpret_cast<double*>(&xv)[1] = Xi[i * LD + k];
            }
        }
        Rout[i + ldr * k] = rv;
        Xout[i + ldx * k] = xv;
    }
}
template <class T>
struct chol_inv_block16_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        chol_inv_block16_body<T>(b, g, a...);
    }
};

// G (n x n, ld n, Hermitian positive definite; DESTROYED) = R^H R;  Rm (upper triangular, ld n) and Xm = R^-1 (ld n), both
// zero below the diagonal (`zeroed`: the caller has cleared them); *flag (device) is raised on a bad pivot.  Diagonal blocks
// of 64 columns in one workgroup each (chol_inv_block16), panels, trailing updates and the merges of R^-1 by MFMA GEMMs.
template <class T>
int chol_inv(qil_context* ctx, T* G, int n, T* Rm, T* Xm, int* flag, bool zeroed = false) {
    constexpr int NBK = 64;
    if (!zeroed) {
        QIL_TRY(qil_dev_zero(ctx, Rm, (size_t)n * n * sizeof(T)));
        QIL_TRY(qil_dev_zero(ctx, Xm, (size_t)n * n * sizeof(T)));
    }
    const int opH = sizeof(T) == 16 ? 2 : 1;
    for (int j0 = 0; j0 < n; j0 += NBK) {
        const int nbj = std::min(NBK, n - j0), rest = n - j0 - nbj;
        QIL_TRY((qil_klaunch<chol_inv_block16_k<T>>(ctx, dim3(1), dim3(256), chol16_lds<T>(), (const T*)(G + j0 + (long long)n * j0), (long long)n, nbj, Rm + j0 + (long long)n * j0, (long long)n, Xm + j0 + (long long)n * j0, (long long)n, 1e-11, flag)));
        if (rest > 0) {
            T* Rjr = Rm + j0 + (long long)n * (j0 + nbj);
            // R(j, rest) = R_jj^-H G(j, rest);   G(rest, rest) -= R(j, rest)^H R(j, rest)
            QIL_TRY(gemm_dispatch<T>(ctx, opH, 0, nbj, rest, nbj, Xm + j0 + (long long)n * j0, n, G + j0 + (long long)n * (j0 + nbj), n, Rjr, n));
            gemm_batch sub;
            sub.subtract = 1;
            QIL_TRY(gemm_dispatch<T>(ctx, opH, 0, rest, rest, nbj, Rjr, n, Rjr, n, G + (j0 + nbj) + (long long)n * (j0 + nbj), n, sub));
        }
    }
    return trtri_merge<T>(ctx, Rm, n, n, Xm, NBK);
}

// The second pass of CholeskyQR2 factors G2 = Q1^H Q1 = I + E with |E| ~ kappa(A)^2 eps.  For |E| this small the factor is
// known to first order without any column chain: R2 = I + U, R2^-1 = I - U with U = striu(E) + diag(E) / 2 (E = U + U^H), the
// neglected terms are O(|E|^2).  One elementwise launch writes both and raises bit 2 of *flag when some |e_ik| exceeds
// `thresh` (the caller then factors G2, which is left intact, properly).
template <class T>
__device__ __forceinline__ void chol_near_identity_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ G, int n, T* __restrict__ R2, T* __restrict__ X2, double thresh, int* __restrict__ flag) {
    bool over = false;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < (long long)n * n; t += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(t % n), k = (int)(t / n);
        T e = G[t], r{}, x{};
        double* ep = reinterpret_cast<double*>(&e);
        if (i == k) {
            ep[0] -= 1.0;
            if (sizeof(T) == 16) ep[1] = 0.0;
        }
        over |= !(abs2_t(e) <= thresh * thresh);
        if (i < k) {
            r = e;
            x = neg_t(e);
        } else if (i == k) {
            reinterpret_cast<double*>(&r)[0] = 1.0 + 0.5 * ep[0];
            reinterpret_cast<double*>(&x)[0] = 1.0 - 0.5 * ep[0];
        }
        R2[t] = r;
        X2[t] = x;
    }
    if (over) atomicOr(flag, 2);
}
template <class T>
struct chol_near_identity_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        chol_near_identity_body<T>(b, g, a...);
    }
};

// A (m x n, m >= n) -> Q in place, R (n x n, ldr; may be null) with positive diagonal.  *done = false: the operand is not
// well enough conditioned (or not positive definite to rounding) -- A and R are untouched, the caller factors it by reflectors.
// orthonormal, rinv: qr_impl's optional out-arguments.
template <class T>
int cholqr2(qil_context* ctx, long long m, long long n, T* A, long long lda, T* R, long long ldr, bool* done, bool* orthonormal,
            void** rinv) {
    *done = false;
    const int opH = sizeof(T) == 16 ? 2 : 1;
    void *g = nullptr, *rx = nullptr, *r2 = nullptr, *x2 = nullptr, *q1 = nullptr;
    auto release = [&]() {
        for (void* b : {g, rx, r2, x2, q1})
            if (b) qil_ctx_free(ctx, b);
    };
    const size_t nn = (size_t)(n * n) * sizeof(T);
    QIL_TRY(qil_ctx_alloc(ctx, nn, &g));
    QIL_TRY(qil_ctx_alloc(ctx, 2 * nn + 256, &rx));              // R1 | X1 | flag: zeroed by ONE launch
    QIL_TRY(qil_ctx_alloc(ctx, nn, &r2));
    QIL_TRY(qil_ctx_alloc(ctx, nn, &x2));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(m * n) * sizeof(T), &q1));
    QIL_TRY(qil_dev_zero(ctx, rx, 2 * nn + 256));
    T *G = static_cast<T*>(g), *R1 = static_cast<T*>(rx), *X1 = R1 + n * n, *R2 = static_cast<T*>(r2), *X2 = static_cast<T*>(x2),
      *Q1 = static_cast<T*>(q1);
    void* fl = static_cast<void*>(X1 + n * n);
    QIL_TRY(gemm_dispatch<T>(ctx, opH, 0, n, n, m, A, lda, A, lda, G, n));
    QIL_TRY(chol_inv<T>(ctx, G, (int)n, R1, X1, (int*)fl, true));
    QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, m, n, n, A, lda, X1, n, Q1, m));
    QIL_TRY(gemm_dispatch<T>(ctx, opH, 0, n, n, m, Q1, m, Q1, m, G, n));
    // second pass: G = I + E; first-order factor while n max |e| <= 3e-8 (|U|^2 below rounding), else the real thing
    // (measured, compress! chi 256 -> 128: 61.8 ms with a second full factorisation, 55.9 ms with this)
    QIL_TRY((qil_klaunch<chol_near_identity_k<T>>(ctx, dim3((unsigned)std::min<long long>((n * n + 255) / 256, 1024)), dim3(256), 0, (const T*)G, (int)n, R2, X2, 3e-8 / (double)n, (int*)fl)));
    int bad = 0;
    QIL_TRY(qil_read_back(ctx, &bad, fl, sizeof(int)));
    const bool first_order = bad == 0;                           // no bad pivot, every |e_ik| <= 3e-8 / n
    const bool refused_first = (bad & 1) != 0;
    if (!(bad & 1) && (bad & 2)) {
        QIL_TRY(qil_dev_zero(ctx, fl, sizeof(int)));
        QIL_TRY(chol_inv<T>(ctx, G, (int)n, R2, X2, (int*)fl));
        QIL_TRY(qil_read_back(ctx, &bad, fl, sizeof(int)));
    }
    if (ctx->qr_report) ctx->qr_report->cholesky = bad ? (refused_first ? 3 : 4) : (first_order ? 1 : 2);
    if (bad) {
        release();
        return QIL_OK;
    }
    QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, m, n, n, Q1, m, X2, n, A, lda));
    if (R) QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, n, n, n, R2, n, R1, n, R, ldr));
    if (R && rinv) {                                             // R^-1 = R1^-1 R2^-1 for the certificate that follows
        QIL_TRY(qil_ctx_alloc(ctx, nn, rinv));
        QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, n, n, n, X1, n, X2, n, static_cast<T*>(*rinv), n));
    }
    release();
    *done = true;
    // Q2 = Q1 (I - U) with Q1^H Q1 = I + E measured, n max |e| <= 3e-8: Q2^H Q2 = I + O(|E|^2), below 1e-15 -- the check that
    // qr_reorthogonalise would run (a Gram product, a max-reduction, a read-back: ~25 us per QR) can only confirm it
    if (orthonormal) *orthonormal = first_order;
    return QIL_OK;
}

// *certified = true iff no singular value of the operand whose thin-QR factor is R can be dropped at `cutoff`.
// rinv: R^-1 (packed, ld k) as CholeskyQR2 left it, or null (then it is computed); freed here.
template <class T>
int certify_no_truncation(qil_context* ctx, const T* R, long long ldr, int k, double cutoff, void* rinv, bool* certified) {
    *certified = false;
    const bool enabled = !(getenv("QIL_SVD_CERT") && atoi(getenv("QIL_SVD_CERT")) == 0);   // tuning aid (read per call: the tests toggle it)
    if (!enabled || !(cutoff > 0.0) || k < 2) {
        if (rinv) qil_ctx_free(ctx, rinv);
        return QIL_OK;
    }
    void *st = nullptr, *xinv = rinv;
    constexpr int NB = 64;
    QIL_TRY(qil_ctx_alloc(ctx, 2 * NB * sizeof(double), &st));
    double hb[2 * NB];
    double h[2];
    auto stats = [&](const T* M, long long ldm) -> int {
        QIL_TRY((qil_klaunch<tri_stats_k<T>>(ctx, dim3(NB), dim3(256), 0, M, ldm, k, 1, (double*)st)));
        QIL_TRY(qil_read_back(ctx, hb, st, sizeof(hb)));
        h[0] = 0;
        h[1] = 1e300;
        for (int b = 0; b < NB; ++b) {          // fixed order
            h[0] += hb[2 * b];
            h[1] = std::min(h[1], hb[2 * b + 1]);
        }
        return QIL_OK;
    };
    QIL_TRY(stats(R, ldr));
    const double fro2 = h[0];
    // sigma_min <= min |r_ii|: a small diagonal entry settles it the other way without inverting anything
    if (!(fro2 > 0.0) || !std::isfinite(fro2) || !(h[1] > 16.0 * cutoff * fro2 * k)) {
        qil_ctx_free(ctx, st);
        if (xinv) qil_ctx_free(ctx, xinv);
        return QIL_OK;
    }
    if (!xinv) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)k * k * sizeof(T), &xinv));
        QIL_TRY(trtri_upper<T>(ctx, R, ldr, k, static_cast<T*>(xinv)));
    }
    QIL_TRY(stats(static_cast<const T*>(xinv), (long long)k));
    qil_ctx_free(ctx, xinv);
    qil_ctx_free(ctx, st);
    const double inv2 = h[0];
    // sigma_min^2 >= 1 / |R^-1|_F^2 must exceed cutoff |R|_F^2; the factor 4 covers the rounding of the inversion
    *certified = std::isfinite(inv2) && inv2 > 0.0 && 4.0 * cutoff * fro2 * inv2 < 1.0;
    if (getenv("QIL_SVD_DEBUG"))
        fprintf(stderr, "[svd-cert] k = %d: cutoff |R|_F^2 |R^-1|_F^2 = %.3e -> %s\n", k, cutoff * fro2 * inv2,
                *certified ? "nothing can be truncated: QR gauge" : "SVD");
    return QIL_OK;
}

// ------------------------------------------------------------------ mid-size SVD with ONE isometric factor
// The gauge sweeps (canonicalize!, compress!, the zip-up) keep only ONE factor of every SVD as a site tensor; the other
// is multiplied into the neighbour.  Then no rotation matrix has to be accumulated: the isometric factor is the
// normalised rotated work matrix itself and the other one is a GEMM with the operand (no division by singular
// values).  Half the LDS per column, half the rotation work per pair, cached squared norms (one wave reduction per pair
// instead of three).

// One outer round of the block tournament without V: workgroup i holds the column blocks (P, Q) of this round in LDS and
// orthogonalises their column pairs in BB (cross pairs; AP: all 2 BB - 1 rounds of all pairs) inner rounds.
// G lanes per column pair (64 = one wave per pair, 32 = two pairs per wave sharing the instruction stream of the rotation),
// KM = rows per lane, BB columns per block; BB G threads.  The inner round is issue-bound (~130 instructions on the wave
// that owns a pair), so it carries no predicates at all: the LDS image of a column has KM G rows, zero beyond m, every lane
// loads and stores all its KM elements, and whether the first round's pairing (AP) applies is a compile-time switch.  In
// cross rounds group `grp` keeps column p = grp of the lower block in registers over all BB inner rounds; only its partner
// travels through LDS.  (Measured, tools/micro/jacobi_round_cost.hip, k = 256 f64: the predicated version spent 1.07 us per
// inner round -- ~40 exec-mask branches -- of a 12.1 us round.)
template <class T, int BB, int KM, int G, bool AP, bool PROF = false>
__device__ __forceinline__ void jacobi_block_round_nov_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ A, long long lda, int m, int n, int nb,
                                                                 int round, double tol, int* __restrict__ rotated,
                                                                 const double* __restrict__ negligible,
                                                                 long long* __restrict__ prof = nullptr,
                                                                 const int* __restrict__ prev = nullptr) {
    // prev: the flags of the PREVIOUS sweep; when that sweep met nothing above the quadratic level the iteration had converged
    // and this launch (issued speculatively by a host that is one sweep ahead of its read-backs) does nothing
    if (prev && !prev[1]) return;
    // PROF (tools/micro/jacobi_round_cost.hip only): shader-clock stamps start / staged / rotated / stored + the 100 MHz clock
    long long st[5];
    if (PROF) {
        st[0] = __builtin_amdgcn_s_memtime();
        st[4] = __builtin_amdgcn_s_memrealtime();
    }
    constexpr int W = 2 * BB;
    constexpr int NT = BB * G;
    constexpr int NWV = NT / 64;                    // waves
    constexpr int ROWS = KM * G;                    // LDS rows of a column (>= m)
    constexpr int KW = ROWS / 64;                   // rows per lane when a whole wave walks a column
    static_assert(ROWS % 64 == 0, "whole waves walk a column");
    constexpr bool CX = sizeof(T) == 16;
    extern __shared__ __attribute__((aligned(16))) char jn_smem[];
    T* As = reinterpret_cast<T*>(jn_smem);          // [W][ROWS]
    double* nr2 = reinterpret_cast<double*>(As + (size_t)ROWS * W);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gl = tid & (G - 1), grp = tid / G;    // lane within the pair's group, group = pair slot
    auto gsum = [](double v) { return group_sum<G>(v); };
    int P, Q;
    {
        const int i = blockIdx.x;
        if (i == 0) {
            P = nb - 1;
            Q = round;
        } else {
            P = (round + i) % (nb - 1);
            Q = (round + nb - 1 - i) % (nb - 1);
        }
        if (P > Q) {
            const int t = P;
            P = Q;
            Q = t;
        }
    }
    auto gcol = [&](int k) { return (k < BB ? P * BB + k : Q * BB + (k - BB)); };
    if (P * BB >= n) return;                               // both blocks are padding
    // staging: the waves share the 2 BB columns (all of a wave's loads in flight at once); squared norms are taken on the way
    constexpr int CPW = W / NWV;
    static_assert(W % NWV == 0, "whole columns per wave");
    {
        T t0[CPW][KW];
#pragma unroll
        for (int cc = 0; cc < CPW; ++cc) {
            const int gc = gcol(wave + cc * NWV);
            const bool cv = gc < n;
            const T* s0 = A + lda * (cv ? gc : 0);
            // rows / columns beyond the matrix: a valid address is loaded and the value multiplied by 0 (a select would be
            // turned into a branch around each load, with a wait inside -- eight serialised round trips to memory)
#pragma unroll
            for (int u = 0; u < KW; ++u) {
                const int r = lane + 64 * u;
                t0[cc][u] = scale_t(s0[r < m ? r : 0], (cv && r < m) ? 1.0 : 0.0);
            }
        }
#pragma unroll
        for (int cc = 0; cc < CPW; ++cc) {
            T* d0 = As + ROWS * (wave + cc * NWV);
            double n0 = 0;
#pragma unroll
            for (int u = 0; u < KW; ++u) {
                d0[lane + 64 * u] = t0[cc][u];
                n0 += abs2_t(t0[cc][u]);
            }
            n0 = wave_sum(n0);
            if (lane == 0) nr2[wave + cc * NWV] = n0;
        }
    }
    __syncthreads();
    if (PROF) st[1] = __builtin_amdgcn_s_memtime();
    const double ng = negligible ? *negligible : 0.0;
    int flags = 0;
    constexpr int nin = AP ? W - 1 : BB;
    T xs[KM];
    double alk = 0;
    if (!AP) {
        const T* ap = As + ROWS * grp;
#pragma unroll
        for (int u = 0; u < KM; ++u) xs[u] = ap[gl + G * u];
        alk = nr2[grp];
    }
    for (int t = 0; t < nin; ++t) {
        int p, q;
        if (AP) {
            if (grp == 0) {
                p = W - 1;
                q = t;
            } else {
                p = t + grp;
                q = t + W - 1 - grp;
                if (p >= W - 1) p -= W - 1;
                if (q >= W - 1) q -= W - 1;
            }
            if (p > q) {
                const int t2 = p;
                p = q;
                q = t2;
            }
        } else {
            p = grp;
            q = grp + t;
            if (q >= BB) q -= BB;
            q += BB;
        }
        if (gcol(p) < n && gcol(q) < n) {
            T* ap = As + ROWS * p;
            T* aq = As + ROWS * q;
            T ys[KM];
#pragma unroll
            for (int u = 0; u < KM; ++u) {
                if (AP) xs[u] = ap[gl + G * u];
                ys[u] = aq[gl + G * u];
            }
            const double al = AP ? nr2[p] : alk, be = nr2[q];
            double gr = 0, gi = 0;
#pragma unroll
            for (int u = 0; u < KM; ++u) dot_parts(xs[u], ys[u], gr, gi);
            if (CX && G == 64) {
                wave_sum2(gr, gi);
            } else {
                gr = gsum(gr);
                if (CX) gi = gsum(gi);
            }
            double c, sr, si, sn, gabs;
            bool big;
            if (!(al < ng || be < ng) && rotation_fast<CX>(al, be, gr, gi, tol, c, sr, si, sn, gabs, big)) {
                flags |= (big || turns_far(al, be, CX ? fma(gr, gr, gi * gi) : gr * gr)) ? 3 : 1;
#pragma unroll
                for (int u = 0; u < KM; ++u) {
                    rotate_pair_sg(xs[u], ys[u], c, sr, si);
                    if (AP) ap[gl + G * u] = xs[u];
                    aq[gl + G * u] = ys[u];
                }
                // |x'|^2 = c^2 al + s^2 be - 2 c s |g|,  |y'|^2 = s^2 al + c^2 be + 2 c s |g|; after strong
                // cancellation the column's norm is taken from the rotated registers instead
                const double cs2 = 2.0 * c * sn * gabs * (be >= al ? 1.0 : -1.0), c2 = c * c, s2 = sn * sn;
                double aln = fma(c2, al, fma(s2, be, -cs2));
                double ben = fma(s2, al, fma(c2, be, cs2));
                if (aln < 0.25 * al || ben < 0.25 * be) {
                    double ea = 0, eb = 0;
#pragma unroll
                    for (int u = 0; u < KM; ++u) {
                        ea += abs2_t(xs[u]);
                        eb += abs2_t(ys[u]);
                    }
                    if (G == 64) {
                        wave_sum2(ea, eb);
                        aln = ea;
                        ben = eb;
                    } else {
                        aln = gsum(ea);
                        ben = gsum(eb);
                    }
                }
                alk = aln;
                if (gl == 0) {
                    if (AP) nr2[p] = aln;
                    nr2[q] = ben;
                }
            }
        }
        __syncthreads();
    }
    if (!AP) {
        T* ap = As + ROWS * grp;
#pragma unroll
        for (int u = 0; u < KM; ++u) ap[gl + G * u] = xs[u];
        __syncthreads();
    }
    if (PROF) st[2] = __builtin_amdgcn_s_memtime();
    if (gl == 0 && flags) {          // plain stores of the same value from every rotating group
        rotated[0] = 1;
        if (flags & 2) rotated[1] = 1;
    }
    for (int kc = wave; kc < W; kc += NWV) {
        const int gc = gcol(kc);
        if (gc >= n) continue;
        T* d = A + lda * gc;
        const T* sp = As + ROWS * kc;
        T t0[KW];
#pragma unroll
        for (int u = 0; u < KW; ++u) t0[u] = sp[lane + 64 * u];
#pragma unroll
        for (int u = 0; u < KW; ++u) {
            const int r = lane + 64 * u;
            if (r < m) d[r] = t0[u];
        }
    }
    if (PROF && tid == 0 && blockIdx.x == 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const long long t3 = __builtin_amdgcn_s_memtime(), r3 = __builtin_amdgcn_s_memrealtime();
        prof[0] += st[1] - st[0];
        prof[1] += st[2] - st[1];
        prof[2] += t3 - st[2];
        prof[3] += r3 - st[4];
        prof[4] += 1;
    }
}
template <class T, int BB, int KM, int G, bool AP, bool PROF = false>
struct jacobi_block_round_nov_k {
    static constexpr int NT = BB * G, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        jacobi_block_round_nov_body<T, BB, KM, G, AP, PROF>(b, g, a...);
    }
};

template <class T, int BB, int KM, int G>
constexpr size_t block_round_nov_lds() {
    return (size_t)2 * BB * KM * G * sizeof(T) + (size_t)2 * BB * sizeof(double);
}

template <class T, int BB, int KM, int G>
int launch_block_round_nov(qil_context* ctx, T* X, long long ldx, int k, int nblk, int round, double tol, int* flag,
                           const double* negl, const int* prev) {
    constexpr size_t lds = block_round_nov_lds<T, BB, KM, G>();
    static_assert(lds <= 156 * 1024, "column blocks must fit the LDS");
    if (round == 0)
        QIL_TRY((qil_klaunch<jacobi_block_round_nov_k<T, BB, KM, G, true>>(ctx, dim3(nblk / 2), dim3(BB * G), lds, X, ldx, k, k, nblk, round, tol, flag, negl, (long long*)nullptr, prev)));
    else
        QIL_TRY((qil_klaunch<jacobi_block_round_nov_k<T, BB, KM, G, false>>(ctx, dim3(nblk / 2), dim3(BB * G), lds, X, ldx, k, k, nblk, round, tol, flag, negl, (long long*)nullptr, prev)));
    return QIL_OK;
}

// ------------------------------------------------------------------ Gram-matrix block round on the matrix cores
// One outer round of the same block tournament, but a block pair is orthogonalised through its Gram matrix instead of column by
// column (the rotation work of the truncate half on v_mfma_f64_16x16x4_f64):
//   1. the W = 2 BB columns of the pair are staged in LDS (rows padded to a multiple of 16, zero filled);
//   2. G = P^H P (W x W) on the matrix cores: 16 x 16 tiles, the K range (the rows) split over the 8 waves, partial tiles
//      summed in a fixed order (deterministic);
//   3. a sweep of TWO-SIDED rotations on G in LDS -- the BB cross pairs per inner round (AP: all pairs of the 2 BB columns,
//      2 BB - 1 inner rounds: the first outer round of a sweep, which also covers the pairs inside a block): threads
//      0 .. BB - 1 derive the rotations from the current diagonal 2 x 2 blocks (no dot products, no reductions), one thread
//      per 2 x 2 block (k1, k2) of G then applies R1^H B R2 in place and the other four waves accumulate J <- J R; two
//      barriers per inner round.  Measured (tools/micro/gram_round_cost.hip, 256 columns f64): ~1 300 cycles per inner
//      round whether every block thread derives its two rotations itself (one barrier, double-buffered G) or they are
//      derived once and shared (two barriers) -- the round is a latency chain (LDS read, rotation, LDS write, barrier, LDS
//      reads, update, barrier), not an issue or bandwidth limit;
//   4. P <- P J on the matrix cores (issued as (J^T tile)(P^T tile) so that every 16 lanes store 128 / 256 contiguous bytes),
//      straight to global memory.
// Convergence flags come from the FRESH Gram matrix (relative to the columns' own norms): flag[0] = some pair above tol,
// flag[1] = some pair above the quadratic-phase level.  prev != nullptr: the flags of the PREVIOUS sweep; when that sweep met
// nothing above the quadratic level the iteration had converged and this launch (issued speculatively by a host that is one
// sweep ahead of its read-backs) does nothing.
template <class T>
struct gram_round_args {
    T* A;
    long long lda;
    int m, n, nb, round;
    double tol;
    int* flag;
    const int* prev;
    const double* negligible;
    long long* prof;            // tools/micro/gram_round_cost.hip only: shader-clock stamps per phase (nullptr in the product)
};

template <class T, int BB>
constexpr size_t gram_round_lds(int m) {
    constexpr int W = 2 * BB, LDG = W + 1, NC = sizeof(T) == 16 ? 2 : 1;
    const int mpad = (m + 15) & ~15;
    return (size_t)W * (mpad + 2) * sizeof(T)             // the column pair
           + (size_t)NC * W * LDG * sizeof(double)        // G, re / im planes
           + (size_t)NC * W * W * sizeof(double)          // J
           + (size_t)8 * NC * 256 * sizeof(double)        // partial Gram tiles of the 8 waves
           + 64;
}

template <class T, int BB, bool AP>
__device__ __forceinline__ void gram_block_round_body(const gram_round_args<T>& a, const unsigned bx) {
    constexpr bool CX = sizeof(T) == 16;
    constexpr int NC = CX ? 2 : 1;
    constexpr int W = 2 * BB, LDG = W + 1;
    constexpr int NTL = W / 16, NT2 = NTL * NTL, KSP = 8 / NT2;      // 16 x 16 tiles of G; waves per tile (K split)
    static_assert(W == 16 || W == 32, "2 x 8 or 2 x 16 columns");
    if (a.prev && !a.prev[1]) return;
    long long st[6] = {0, 0, 0, 0, 0, 0};
    if (a.prof) st[0] = __builtin_amdgcn_s_memtime();
    const int m = a.m, n = a.n, nb = a.nb, round = a.round;
    const int mpad = (m + 15) & ~15, LDR = mpad + 2;
    extern __shared__ __attribute__((aligned(16))) char gr_smem[];
    T* Xs = reinterpret_cast<T*>(gr_smem);                           // [W][LDR]
    double* Gb = reinterpret_cast<double*>(Xs + (size_t)W * LDR);    // [NC][W * LDG]
    double* Jm = Gb + NC * W * LDG;                                  // [NC][W * W], J[c][j] at c * W + j
    double* Pp = Jm + NC * W * W;                                    // [8][NC][256]
    int* sflag = reinterpret_cast<int*>(Pp + 8 * NC * 256);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int P, Q;
    {
        const int i = (int)bx;
        if (i == 0) {
            P = nb - 1;
            Q = round;
        } else {
            P = (round + i) % (nb - 1);
            Q = (round + nb - 1 - i) % (nb - 1);
        }
        if (nb == 2) {
            P = 0;
            Q = 1;
        }
        if (P > Q) {
            const int t = P;
            P = Q;
            Q = t;
        }
    }
    if (P * BB >= n) return;                                         // both blocks are padding
    auto gcol = [&](int k) { return (k < BB ? P * BB + k : Q * BB + (k - BB)); };
    if (tid == 0) *sflag = 0;
    // ---- 1. staging (ALL of a wave's loads in flight before the first LDS store -- a column per trip pays one memory
    // latency per column; rows / columns beyond the matrix: clamped address, value times 0)
    {
        constexpr int CPW = W / 8;                                   // columns per wave
        for (int r0 = 0; r0 < mpad; r0 += 256) {
            T t0[CPW][4];
#pragma unroll
            for (int cc = 0; cc < CPW; ++cc) {
                const int gc = gcol(wave + 8 * cc);
                const bool cv = gc < n;
                const T* s0 = a.A + a.lda * (cv ? gc : 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = r0 + lane + 64 * u;
                    t0[cc][u] = scale_t(s0[r < m ? r : 0], (cv && r < m) ? 1.0 : 0.0);
                }
            }
#pragma unroll
            for (int cc = 0; cc < CPW; ++cc) {
                T* d0 = Xs + (size_t)LDR * (wave + 8 * cc);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = r0 + lane + 64 * u;
                    if (r < mpad) d0[r] = t0[cc][u];
                }
            }
        }
    }
    __syncthreads();
    if (a.prof) st[1] = __builtin_amdgcn_s_memtime();
    // ---- 2. G = X^H X: wave -> (tile, K slice)
    {
        const int tile = wave / KSP, ks0 = wave % KSP;
        const int ti = tile / NTL, tj = tile % NTL;
        const int li = lane & 15, lk = lane >> 4;
        d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
        const T* xa = Xs + (size_t)LDR * (16 * ti + li) + lk;
        const T* xb = Xs + (size_t)LDR * (16 * tj + li) + lk;
        const int nks = mpad / 4;
        d4 rr2 = {0, 0, 0, 0}, ii2 = {0, 0, 0, 0}, ri2 = {0, 0, 0, 0};   // second accumulator set: no dependent MFMA chain
        int ks = ks0;
        // eight K steps per trip: all sixteen fragment reads are issued before the first MFMA (one LDS latency per trip
        // instead of one per step: 6 800 -> see tools/micro/gram_round_cost.hip), two accumulator sets alternate
        constexpr int UNR = 8;
        for (; ks + (UNR - 1) * KSP < nks; ks += UNR * KSP) {
            T av[UNR], bv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                av[u] = xa[4 * (ks + u * KSP)];
                bv[u] = xb[4 * (ks + u * KSP)];
            }
#pragma unroll
            for (int u = 0; u < UNR; u += 2) {
                if constexpr (CX) {
                    // G = (ar - i ai)^T (br + i bi):  re = ar br + ai bi,  im = ar bi - ai br
                    rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].re, bv[u].re, rr, 0, 0, 0);
                    rr2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1].re, bv[u + 1].re, rr2, 0, 0, 0);
                    rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].im, bv[u].im, rr, 0, 0, 0);
                    rr2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1].im, bv[u + 1].im, rr2, 0, 0, 0);
                    ri = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].re, bv[u].im, ri, 0, 0, 0);
                    ri2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1].re, bv[u + 1].im, ri2, 0, 0, 0);
                    ii = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].im, bv[u].re, ii, 0, 0, 0);
                    ii2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1].im, bv[u + 1].re, ii2, 0, 0, 0);
                } else {
                    rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], rr, 0, 0, 0);
                    rr2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1], bv[u + 1], rr2, 0, 0, 0);
                }
            }
        }
        for (; ks < nks; ks += KSP) {
            const T av = xa[4 * ks], bv = xb[4 * ks];
            if constexpr (CX) {
                rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av.re, bv.re, rr, 0, 0, 0);
                rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av.im, bv.im, rr, 0, 0, 0);
                ri = __builtin_amdgcn_mfma_f64_16x16x4f64(av.re, bv.im, ri, 0, 0, 0);
                ii = __builtin_amdgcn_mfma_f64_16x16x4f64(av.im, bv.re, ii, 0, 0, 0);
            } else {
                rr = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, rr, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rr[r] += rr2[r];
            ii[r] += ii2[r];
            ri[r] += ri2[r];
        }
        double* pw = Pp + (size_t)wave * NC * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pw[(lk + 4 * r) * 16 + li] = rr[r];                      // row i = lk + 4 r, col j = li of the tile
            if constexpr (CX) pw[256 + (lk + 4 * r) * 16 + li] = ri[r] - ii[r];
        }
    }
    __syncthreads();
    double* G0 = Gb;
    for (int t = tid; t < NT2 * 256; t += 512) {
        const int tile = t >> 8, e = t & 255, i = e >> 4, j = e & 15;
        const int ti = tile / NTL, tj = tile % NTL;
        double vr = 0, vi = 0;
#pragma unroll
        for (int k = 0; k < KSP; ++k) {
            vr += Pp[(size_t)(tile * KSP + k) * NC * 256 + e];
            if constexpr (CX) vi += Pp[(size_t)(tile * KSP + k) * NC * 256 + 256 + e];
        }
        G0[(16 * ti + i) * LDG + 16 * tj + j] = vr;
        if constexpr (CX) G0[W * LDG + (16 * ti + i) * LDG + 16 * tj + j] = vi;
    }
    for (int t = tid; t < W * W; t += 512) {
        Jm[t] = (t / W == t % W) ? 1.0 : 0.0;
        if constexpr (CX) Jm[W * W + t] = 0.0;
    }
    __syncthreads();
    if (a.prof) st[2] = __builtin_amdgcn_s_memtime();
    const double ng = a.negligible ? *a.negligible : 0.0;
    // ---- convergence flags from the fresh Gram matrix (this visit's pairs)
    {
        int fl = 0;
        for (int t = tid; t < W * W; t += 512) {
            const int r = t % W, c = t / W;
            const bool mine = AP ? (r < c) : (r < BB && c >= BB);
            if (!mine) continue;
            const double al = G0[r * LDG + r], be = G0[c * LDG + c];
            if (al < ng || be < ng) continue;
            double g2 = G0[r * LDG + c] * G0[r * LDG + c];
            if constexpr (CX) g2 = fma(G0[W * LDG + r * LDG + c], G0[W * LDG + r * LDG + c], g2);
            const double ab = al * be;
            if (g2 > a.tol * a.tol * ab && g2 != 0.0) fl |= turns_far(al, be, g2) ? 3 : 1;
            if (g2 > kQuadraticOff * kQuadraticOff * ab) fl |= 2;
        }
        if (fl) atomicOr(sflag, fl);
    }
    __syncthreads();
    const int fl_all = *sflag;
    if (!(fl_all & 1)) return;                                       // nothing to rotate: the columns stay as they are
    if (tid == 0) {
        a.flag[0] = 1;
        if (fl_all & 2) a.flag[1] = 1;
    }
    if (a.prof) st[3] = __builtin_amdgcn_s_memtime();
    // ---- 3. two-sided rotations on G (threads 0 .. BB^2 - 1: one 2 x 2 block each), J <- J R (threads 256 ..)
    constexpr int nin = AP ? W - 1 : BB;
    auto pair_of = [&](int k, int t, int& p, int& q) {
        if (AP) {
            if (k == 0) {
                p = W - 1;
                q = t;
            } else {
                p = t + k;
                q = t + W - 1 - k;
                if (p >= W - 1) p -= W - 1;
                if (q >= W - 1) q -= W - 1;
            }
            if (p > q) {
                const int t2 = p;
                p = q;
                q = t2;
            }
        } else {
            p = k;
            q = k + t;
            if (q >= BB) q -= BB;
            q += BB;
        }
    };
    auto rot_of = [&](const double* G, int p, int q, double& c, double& sr, double& si) {
        const double al = G[p * LDG + p], be = G[q * LDG + q];
        const double gr = G[p * LDG + q], gi = CX ? G[W * LDG + p * LDG + q] : 0.0;
        double sabs, gabs;
        bool big;
        if (al < ng || be < ng || !rotation_fast<CX>(al, be, gr, gi, a.tol, c, sr, si, sabs, gabs, big)) {
            c = 1.0;
            sr = 0.0;
            si = 0.0;
        }
    };
    // Every pair's rotation is derived ONCE (threads 0 .. BB - 1, from the current diagonal 2 x 2 blocks) and handed to the
    // block / J threads through LDS: two barriers per inner round.
    double* rotc = Pp;                                               // the partial-tile area is free again: c, sr, si per pair
    double* rotr = Pp + BB;
    double* roti = Pp + 2 * BB;
    int* rotp = reinterpret_cast<int*>(Pp + 3 * BB);                 // and its two columns
    int* rotq = rotp + BB;
    const bool gthr = tid < BB * BB;
    const int k1 = tid % BB, k2 = (tid / BB) % BB;                   // block (k1, k2) of G
    const bool jthr = tid >= 256 && tid < 256 + BB * (W / 2);
    const int jk = (tid - 256) % BB, ji = ((tid - 256) / BB) * 2;    // pair jk, rows ji, ji + 1 of J
    double* G = Gb;                                                  // updated in place: every entry belongs to one block thread
    for (int t = 0; t < nin; ++t) {
        if (tid < BB) {
            int p, q;
            pair_of(tid, t, p, q);
            double c, sr, si;
            rot_of(G, p, q, c, sr, si);
            rotc[tid] = c;
            rotr[tid] = sr;
            if constexpr (CX) roti[tid] = si;
            rotp[tid] = p;
            rotq[tid] = q;
        }
        __syncthreads();
        if (gthr) {
            const int p1 = rotp[k1], q1 = rotq[k1], p2 = rotp[k2], q2 = rotq[k2];
            const double c1 = rotc[k1], s1r = rotr[k1], c2 = rotc[k2], s2r = rotr[k2];
            const double s1i = CX ? roti[k1] : 0.0, s2i = CX ? roti[k2] : 0.0;
            // B = [[G p1p2, G p1q2], [G q1p2, G q1q2]]
            const double b00r = G[p1 * LDG + p2], b01r = G[p1 * LDG + q2], b10r = G[q1 * LDG + p2], b11r = G[q1 * LDG + q2];
            if constexpr (CX) {
                double* Gi = G + W * LDG;
                const double b00i = Gi[p1 * LDG + p2], b01i = Gi[p1 * LDG + q2], b10i = Gi[q1 * LDG + p2], b11i = Gi[q1 * LDG + q2];
                // columns: M = B R2:  M[:,0] = c2 B[:,0] - conj(s2) B[:,1];  M[:,1] = s2 B[:,0] + c2 B[:,1]
                const double m00r = c2 * b00r - (s2r * b01r + s2i * b01i), m00i = c2 * b00i - (s2r * b01i - s2i * b01r);
                const double m10r = c2 * b10r - (s2r * b11r + s2i * b11i), m10i = c2 * b10i - (s2r * b11i - s2i * b11r);
                const double m01r = (s2r * b00r - s2i * b00i) + c2 * b01r, m01i = (s2r * b00i + s2i * b00r) + c2 * b01i;
                const double m11r = (s2r * b10r - s2i * b10i) + c2 * b11r, m11i = (s2r * b10i + s2i * b10r) + c2 * b11i;
                // rows: R1^H M:  row0 = c1 M0 - s1 M1;  row1 = conj(s1) M0 + c1 M1
                G[p1 * LDG + p2] = c1 * m00r - (s1r * m10r - s1i * m10i);
                Gi[p1 * LDG + p2] = c1 * m00i - (s1r * m10i + s1i * m10r);
                G[p1 * LDG + q2] = c1 * m01r - (s1r * m11r - s1i * m11i);
                Gi[p1 * LDG + q2] = c1 * m01i - (s1r * m11i + s1i * m11r);
                G[q1 * LDG + p2] = (s1r * m00r + s1i * m00i) + c1 * m10r;
                Gi[q1 * LDG + p2] = (s1r * m00i - s1i * m00r) + c1 * m10i;
                G[q1 * LDG + q2] = (s1r * m01r + s1i * m01i) + c1 * m11r;
                Gi[q1 * LDG + q2] = (s1r * m01i - s1i * m01r) + c1 * m11i;
            } else {
                const double m00 = fma(c2, b00r, -s2r * b01r), m01 = fma(s2r, b00r, c2 * b01r);
                const double m10 = fma(c2, b10r, -s2r * b11r), m11 = fma(s2r, b10r, c2 * b11r);
                G[p1 * LDG + p2] = fma(c1, m00, -s1r * m10);
                G[p1 * LDG + q2] = fma(c1, m01, -s1r * m11);
                G[q1 * LDG + p2] = fma(s1r, m00, c1 * m10);
                G[q1 * LDG + q2] = fma(s1r, m01, c1 * m11);
            }
        } else if (jthr) {
            const int p = rotp[jk], q = rotq[jk];
            const double c = rotc[jk], sr = rotr[jk], si = CX ? roti[jk] : 0.0;
            if (sr != 0.0 || si != 0.0) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int i = ji + u;
                    if constexpr (CX) {
                        c64 x{Jm[i * W + p], Jm[W * W + i * W + p]}, y{Jm[i * W + q], Jm[W * W + i * W + q]};
                        rotate_pair_sg(x, y, c, sr, si);
                        Jm[i * W + p] = x.re;
                        Jm[W * W + i * W + p] = x.im;
                        Jm[i * W + q] = y.re;
                        Jm[W * W + i * W + q] = y.im;
                    } else {
                        double x = Jm[i * W + p], y = Jm[i * W + q];
                        rotate_pair_sg(x, y, c, sr, si);
                        Jm[i * W + p] = x;
                        Jm[i * W + q] = y;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (a.prof) st[4] = __builtin_amdgcn_s_memtime();
    // ---- 4. X <- X J (as (J^T)(X^T): D[j][r]), wave -> row tiles
    {
        const int li = lane & 15, lk = lane >> 4;
        double jr[NTL][W / 4], jim[NTL][W / 4];
#pragma unroll
        for (int tj = 0; tj < NTL; ++tj)
#pragma unroll
            for (int ks = 0; ks < W / 4; ++ks) {
                jr[tj][ks] = Jm[(4 * ks + lk) * W + 16 * tj + li];
                jim[tj][ks] = CX ? Jm[W * W + (4 * ks + lk) * W + 16 * tj + li] : 0.0;
            }
        for (int rt = wave; rt < mpad / 16; rt += 8) {
            d4 rr[NTL], ii[NTL], ri[NTL];
#pragma unroll
            for (int tj = 0; tj < NTL; ++tj) rr[tj] = ii[tj] = ri[tj] = d4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < W / 4; ++ks) {
                const T xv = Xs[(size_t)LDR * (4 * ks + lk) + 16 * rt + li];
#pragma unroll
                for (int tj = 0; tj < NTL; ++tj) {
                    if constexpr (CX) {
                        rr[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(jr[tj][ks], xv.re, rr[tj], 0, 0, 0);
                        ii[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(jim[tj][ks], xv.im, ii[tj], 0, 0, 0);
                        ri[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(jim[tj][ks], xv.re, ri[tj], 0, 0, 0);
                        ri[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(jr[tj][ks], xv.im, ri[tj], 0, 0, 0);
                    } else {
                        rr[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(jr[tj][ks], xv, rr[tj], 0, 0, 0);
                    }
                }
            }
            const int r = 16 * rt + li;
#pragma unroll
            for (int tj = 0; tj < NTL; ++tj)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int gc = gcol(16 * tj + lk + 4 * q4);
                    if (r < m && gc < n) {
                        if constexpr (CX)
                            a.A[a.lda * gc + r] = T{rr[tj][q4] - ii[tj][q4], ri[tj][q4]};
                        else
                            a.A[a.lda * gc + r] = rr[tj][q4];
                    }
                }
        }
    }
    if (a.prof && tid == 0 && bx == 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st[5] = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < 5; ++i) a.prof[i] += st[i + 1] - st[i];
        a.prof[5] += 1;
    }
}

template <class T, int BB, bool AP>
struct gram_block_round_k {
    static constexpr int NT = 512, MINW = 1;
    static __device__ __forceinline__ void run(const uint3 b, const uint3, gram_round_args<T> a) { gram_block_round_body<T, BB, AP>(a, b.x); }
};

template <class T, int BB>
int launch_gram_round(qil_context* ctx, T* X, long long ldx, int k, int nblk, int round, double tol, int* flag, const int* prev,
                      const double* negl) {
    const size_t lds = gram_round_lds<T, BB>(k);
    gram_round_args<T> a{X, ldx, k, k, nblk, round, tol, flag, prev, negl, nullptr};
    if (round == 0) return qil_klaunch<gram_block_round_k<T, BB, true>>(ctx, dim3(nblk / 2), dim3(512), lds, a);
    return qil_klaunch<gram_block_round_k<T, BB, false>>(ctx, dim3(nblk / 2), dim3(512), lds, a);
}


// B (p x q, ldb; destroyed) = Uiso diag(S) V^H:  Uiso (p x k, k = min(p, q)) orthonormal columns sorted by descending
// singular value, S on the host, SVh (k x q) = diag(S) V^H.  Serves 97 <= k < 640 (and smaller k whose general path would not be LDS-resident) with the columns in LDS;
// *handled = 0 (nothing touched beyond B's contents being intact) sends the caller to the general svd_impl.
template <class T>
int svd_impl(qil_context* ctx, long long m, long long n, T* A, long long lda, T* U, long long ldu, double* S_host, T* Vh,
             long long ldvh, double negl_rel);

// svd_left_mid's route for rank-deficient triangular factors (see there): R (k x k, ld k) = thin-QR factor of the tall operand,
// Q (p x k, ldq) its basis, Xw (k x k workspace).  Rows of R are dropped while their weight stays below deflate |R|_F^2.
// *done = 0: too few negligible rows, nothing written.
template <class T>
int svd_left_mid(qil_context* ctx, long long p, long long q, T* B, long long ldb, T* Uiso, long long ldu, double* S_host,
                 T* SVh, long long ldsvh, double negl_rel, int* handled, double cert_cutoff, double deflate);
template <class T>
int svd_left_deflated(qil_context* ctx, long long p, long long k, const T* Q, long long ldq, const T* R, T* Xw, T* Uiso,
                      long long ldu, double* S_host, T* SVh, long long ldsvh, double negl_rel, double deflate, bool dbg, int* done) {
    *done = 0;
    const int dtype = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    const unsigned gk = (unsigned)std::min<long long>((k * k + 255) / 256, 65536);
    // the rows of R as the columns of Xw = R^H, their squared norms to the host
    void* nrm = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)k * sizeof(double), &nrm));
    QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3(gk), dim3(256), 0, R, k, k, k, Xw, k)));
    QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)k), dim3(256), 0, (const T*)Xw, k, k, (double*)nrm)));
    std::vector<double> rn((size_t)k);
    const int rst = qil_read_back(ctx, rn.data(), nrm, (size_t)k * sizeof(double));
    qil_ctx_free(ctx, nrm);
    QIL_TRY(rst);
    double total = 0.0;
    for (double& v : rn) {
        v *= v;                                                  // (col_norms_k returns norms)
        total += v;
    }
    std::vector<int> order((size_t)k);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rn[(size_t)a] < rn[(size_t)b]; });
    std::vector<char> drop((size_t)k, 0);
    double acc = 0.0;
    long long ndrop = 0;
    for (int j : order) {
        if (!(acc + rn[(size_t)j] <= deflate * total)) break;
        acc += rn[(size_t)j];
        drop[(size_t)j] = 1;
        ++ndrop;
    }
    const long long r = k - ndrop;
    if (dbg) fprintf(stderr, "[svd-left] deflation: %lld of %lld rows of R carry all but %.1e of the weight\n", r, k, total > 0 ? acc / total : 0.0);
    // (measured on the exact compress! of the bond-1008 zT product, deflating when at most 0.6 / 0.75 / 0.9 / 0.97 / 0.995 of the
    // rows stay: 279 / 291 / 268 / 252 / 252 ms, 295 without: even 10 % negligible rows are worth it -- what goes is the
    // degenerate cluster the sweeps crawl on)
    if (r < 1 || (double)r > 0.97 * (double)k) return QIL_OK;
    std::vector<int> keep;
    keep.reserve((size_t)r);
    for (long long j = 0; j < k; ++j)
        if (!drop[(size_t)j]) keep.push_back((int)j);            // in the original order
    void *hp = nullptr, *dp = nullptr, *bk = nullptr, *uk = nullptr, *svk = nullptr, *qk = nullptr;
    auto release = [&]() {
        for (void* b : {bk, uk, svk, qk})
            if (b) qil_ctx_free(ctx, b);
    };
    int slot = -1;
    QIL_TRY(qil_stage_acquire(ctx, (size_t)r * sizeof(int), &hp, &dp, &slot));
    memcpy(hp, keep.data(), (size_t)r * sizeof(int));
    QIL_TRY(qil_stage_push(ctx, slot, (size_t)r * sizeof(int)));
    const int* keepd = static_cast<const int*>(dp);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(r * k) * sizeof(T), &bk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(r * r) * sizeof(T), &uk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(r * k) * sizeof(T), &svk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(p * r) * sizeof(T), &qk));
    T *Bk = static_cast<T*>(bk), *Uk = static_cast<T*>(uk), *SVk = static_cast<T*>(svk), *Qk = static_cast<T*>(qk);
    // Bk = R[K, :] (r x k) = (Xw[:, K])^H;  Qk = Q[:, K]
    QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3(gk), dim3(256), 0, (const T*)Xw, k, k, keepd, (const double*)nullptr, Bk, r, (int)r, 1)));
    QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3((unsigned)std::min<long long>((p * r + 255) / 256, 65536)), dim3(256), 0, Q, ldq, p, keepd, (const double*)nullptr, Qk, p, (int)r, 0)));
    qil_stage_commit(ctx, slot);
    // one-factor SVD of the wide block: Bk = Uk diag(S) V^H, SVk = diag(S) V^H
    int h2 = 0;
    int st = svd_left_mid<T>(ctx, r, k, Bk, r, Uk, r, S_host, SVk, r, negl_rel, &h2, 0.0, deflate);
    if (st == QIL_OK && !h2) {                                   // outside the one-factor routine's range: the general SVD
        st = svd_impl<T>(ctx, r, k, Bk, r, Uk, r, S_host, SVk, r, negl_rel);
        if (st == QIL_OK) st = qil_dev_scale(ctx, dtype, 0, r, k, SVk, r, S_host);
    }
    if (st != QIL_OK) {
        release();
        return st;
    }
    for (long long j = r; j < k; ++j) S_host[j] = 0.0;
    // Uiso = [Q[:, K] Uk, 0],  S V^H = [SVk; 0]
    st = gemm_dispatch<T>(ctx, 0, 0, p, r, r, Qk, p, Uk, r, Uiso, ldu);
    if (st == QIL_OK) st = qil_dev_zero2d(ctx, Uiso + ldu * r, (size_t)ldu * sizeof(T), (size_t)p * sizeof(T), (size_t)(k - r));
    if (st == QIL_OK) st = qil_dev_zero2d(ctx, SVh, (size_t)ldsvh * sizeof(T), (size_t)k * sizeof(T), (size_t)k);
    if (st == QIL_OK) st = qil_dev_copy2d(ctx, SVh, (size_t)ldsvh * sizeof(T), SVk, (size_t)r * sizeof(T), (size_t)r * sizeof(T), (size_t)k);
    release();
    QIL_TRY(st);
    *done = 1;
    return QIL_OK;
}

// The same for a WIDE operand B (k x q, k < q), B^H = Q R: B = X Q^H with X = R^H (k x k), whose COLUMNS are the rows of R.
// Negligible columns of X are dropped (exactly their weight), X[:, K] = U' S' V'^H (tall, k x r) gives U = U' and
// S V^H = (S' V'^H) Q[:, K]^H.  Q (q x k, ldq); X is left intact.  *done = 0: nothing written.
template <class T>
int svd_left_deflated_wide(qil_context* ctx, long long k, long long q, const T* Q, long long ldq, const T* X, T* Uiso, long long ldu,
                           double* S_host, T* SVh, long long ldsvh, double negl_rel, double deflate, bool dbg, int* done) {
    *done = 0;
    const int dtype = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    void* nrm = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)k * sizeof(double), &nrm));
    QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)k), dim3(256), 0, X, k, k, (double*)nrm)));
    std::vector<double> rn((size_t)k);
    const int rst = qil_read_back(ctx, rn.data(), nrm, (size_t)k * sizeof(double));
    qil_ctx_free(ctx, nrm);
    QIL_TRY(rst);
    double total = 0.0;
    for (double& v : rn) {
        v *= v;
        total += v;
    }
    std::vector<int> order((size_t)k);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rn[(size_t)a] < rn[(size_t)b]; });
    std::vector<char> drop((size_t)k, 0);
    double acc = 0.0;
    long long ndrop = 0;
    for (int j : order) {
        if (!(acc + rn[(size_t)j] <= deflate * total)) break;
        acc += rn[(size_t)j];
        drop[(size_t)j] = 1;
        ++ndrop;
    }
    const long long r = k - ndrop;
    if (dbg) fprintf(stderr, "[svd-left] deflation (wide): %lld of %lld rows of R carry all but %.1e of the weight\n", r, k, total > 0 ? acc / total : 0.0);
    if (r < 1 || (double)r > 0.97 * (double)k) return QIL_OK;
    std::vector<int> keep;
    keep.reserve((size_t)r);
    for (long long j = 0; j < k; ++j)
        if (!drop[(size_t)j]) keep.push_back((int)j);
    void *hp = nullptr, *dp = nullptr, *xk = nullptr, *uk = nullptr, *svk = nullptr, *qk = nullptr;
    auto release = [&]() {
        for (void* b : {xk, uk, svk, qk})
            if (b) qil_ctx_free(ctx, b);
    };
    int slot = -1;
    QIL_TRY(qil_stage_acquire(ctx, (size_t)r * sizeof(int), &hp, &dp, &slot));
    memcpy(hp, keep.data(), (size_t)r * sizeof(int));
    QIL_TRY(qil_stage_push(ctx, slot, (size_t)r * sizeof(int)));
    const int* keepd = static_cast<const int*>(dp);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * r) * sizeof(T), &xk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * r) * sizeof(T), &uk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(r * r) * sizeof(T), &svk));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(q * r) * sizeof(T), &qk));
    T *Xk = static_cast<T*>(xk), *Uk = static_cast<T*>(uk), *SVk = static_cast<T*>(svk), *Qk = static_cast<T*>(qk);
    QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3((unsigned)std::min<long long>((k * r + 255) / 256, 65536)), dim3(256), 0, X, k, k, keepd, (const double*)nullptr, Xk, k, (int)r, 0)));
    QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3((unsigned)std::min<long long>((q * r + 255) / 256, 65536)), dim3(256), 0, Q, ldq, q, keepd, (const double*)nullptr, Qk, q, (int)r, 0)));
    qil_stage_commit(ctx, slot);
    int h2 = 0;
    int st = svd_left_mid<T>(ctx, k, r, Xk, k, Uk, k, S_host, SVk, r, negl_rel, &h2, 0.0, deflate);
    if (st == QIL_OK && !h2) {
        st = svd_impl<T>(ctx, k, r, Xk, k, Uk, k, S_host, SVk, r, negl_rel);
        if (st == QIL_OK) st = qil_dev_scale(ctx, dtype, 0, r, r, SVk, r, S_host);
    }
    if (st != QIL_OK) {
        release();
        return st;
    }
    for (long long j = r; j < k; ++j) S_host[j] = 0.0;
    st = qil_dev_zero2d(ctx, Uiso, (size_t)ldu * sizeof(T), (size_t)k * sizeof(T), (size_t)k);
    if (st == QIL_OK) st = qil_dev_copy2d(ctx, Uiso, (size_t)ldu * sizeof(T), Uk, (size_t)k * sizeof(T), (size_t)k * sizeof(T), (size_t)r);
    if (st == QIL_OK) st = qil_dev_zero2d(ctx, SVh, (size_t)ldsvh * sizeof(T), (size_t)k * sizeof(T), (size_t)q);
    if (st == QIL_OK) st = gemm_dispatch<T>(ctx, 0, 2, r, q, r, SVk, r, Qk, q, SVh, ldsvh);
    release();
    QIL_TRY(st);
    *done = 1;
    return QIL_OK;
}

template <class T>
int svd_left_mid(qil_context* ctx, long long p, long long q, T* B, long long ldb, T* Uiso, long long ldu, double* S_host,
                 T* SVh, long long ldsvh, double negl_rel, int* handled, double cert_cutoff, double deflate) {
    *handled = 0;
    const long long k = std::min(p, q);
    if (k < 17 || k >= 640) return QIL_OK;
    static const long long fused_below = 49;   // (97 -> 49: compress! chi 64 -> 32 31.6 -> 28 ms, 128 -> 64 52.6 -> 50 ms)
    if (k < fused_below) {
        // small operands: the single-workgroup iteration of the general path (operand and V in LDS, no launches) wins
        // whenever it fits; where it does not (complex 2 chi x chi sites with chi > 64, long rows) that path falls back to V
        // in global memory (1.1 ms per SVD) or to per-round launches that carry V, and the one-factor route is 2x faster
        const long long rows = std::max(p, q);
        const size_t lds_av = (size_t)((rows | 1) * k + (k | 1) * k) * sizeof(T);
        if (lds_av <= 150 * 1024 && rows * k <= (1LL << 19)) return QIL_OK;
    }
    // Block / group shape.  A sweep over n columns is n - 1 inner rounds of n / 2 pairs whatever the blocking; an inner round
    // is issue-bound on the wave that owns a pair, and every outer round pays a launch plus the staging of its columns: one
    // wave per pair, blocks of 8 columns, 512 threads = two waves per SIMD hiding each other's LDS and dependent-issue
    // latency.  (Two pairs per wave on 16-column blocks -- half the outer rounds, the rotation chain paid once per two pairs --
    // was measured equal in r02, 126 vs 124 ms, and removed.)
    const int km = (int)((k + 63) / 64);             // rows per lane, one wave per column
    int bb = 8;
    // Gram-matrix block rounds on the matrix cores (gram_block_round) whenever a block pair and its Gram workspace fit one
    // CU's LDS: 2 x 16 columns, else 2 x 8
    // (measured, compress! on 24 sites: f64 chi 256 -> 128 69.9 ms with the Gram rounds, 70.4 ms with the vector rounds; c64 107
    // against 103 ms -- a Gram round of 2 x 16 columns takes 20 us where two vector rounds of 2 x 8 take 18, both bound by the
    // latency of the rotation rounds, tools/micro/gram_round_cost.hip -- so complex operands keep the vector rounds)
    // (r04 measured the c64 Gram rounds once more -- exact compress!(apply) 302 against 272 ms, chi 256 equal -- and r05 removed
    // the QIL_SVD_GRAM switch with them: f64 operands take the Gram rounds, complex ones the vector rounds)
    int gbb = 0;
    if (sizeof(T) == 8) {
        if (gram_round_lds<T, 16>((int)k) <= 160 * 1024) gbb = 16;
        else if (gram_round_lds<T, 8>((int)k) <= 160 * 1024) gbb = 8;
    }
    if (!gbb && (size_t)16 * km * 64 * sizeof(T) + 128 > 150 * 1024) return QIL_OK;
    if (gbb) bb = gbb;
    const bool dbg = getenv("QIL_SVD_DEBUG") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        (void)qil_stream_sync(ctx);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[svd-left] %lld x %lld: %s %.2f ms\n", p, q, what,
                std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    const bool tall = p >= q;
    qil_progress_phase(ctx, 1);                              // lock-step batches: QR < grading / second QR < certificate < sweeps < factors
    const int cj = sizeof(T) == 16 ? 2 : 1;
    const unsigned gk = (unsigned)std::min<long long>((k * k + 255) / 256, 65536);
    void *rbuf = nullptr, *xbuf = nullptr, *bh = nullptr, *flag = nullptr, *nrm = nullptr, *negl = nullptr, *wbuf = nullptr;
    void* permbuf = nullptr;                          // [q] column permutation, [q] its inverse (device), see "sorted by norm" below
    void* rinv = nullptr;                             // R^-1 from CholeskyQR2 for the certificate (tall operands, cert_cutoff > 0)
    auto release = [&]() {
        for (void* b : {rbuf, xbuf, bh, flag, nrm, negl, wbuf, permbuf, rinv})
            if (b) qil_ctx_free(ctx, b);
        permbuf = nullptr;
        rinv = nullptr;
    };
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * k) * sizeof(T), &rbuf));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * k) * sizeof(T), &xbuf));
    T* R = static_cast<T*>(rbuf);
    T* X = static_cast<T*>(xbuf);
    T* Qm = nullptr;
    long long ldq = 0, qrows = 0;
    // r06: the COLUMNS OF B ARE SORTED BY NORM (descending) before the QR.  The unpivoted CholeskyQR leaves a triangular factor
    // whose rows are in whatever order the columns came, and one-sided Jacobi on it needs 11 sweeps on average on the graded
    // operands of a truncating sweep (zT product, n = 24: 40 mid-size SVDs, 8 ... 16 sweeps each).  With the columns in
    // descending norm order the QR is the first-order image of a column-pivoted one (Drmac-Veselic preconditioning): the same
    // operands take 6 ... 8 sweeps (numpy model of this iteration on the matrices of that sweep: 15.9 -> 7.0; a true pivoted QR
    // gives 6.2).  Cost: one norm kernel, one small read-back, one gather; B P = Q R, so U is untouched and S V^H = (W^H R) P^T
    // has its columns put back at every exit below.
    bool permuted = false;
    auto put_back_columns = [&](T* Mx, long long ldm, long long rows) -> int {       // Mx[:, perm[j]] <- Mx[:, j]
        if (!permuted) return QIL_OK;
        void* tmp = nullptr;
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(rows * q) * sizeof(T), &tmp));
        const unsigned g = (unsigned)std::min<long long>((rows * q + 1023) / 1024, 4096);
        QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3(g), dim3(1024), 0, (const T*)Mx, ldm, rows, static_cast<const int*>(permbuf) + q,
                                                  (const double*)nullptr, static_cast<T*>(tmp), rows, (int)q, 0)));
        QIL_TRY(qil_dev_copy2d(ctx, Mx, (size_t)ldm * sizeof(T), tmp, (size_t)rows * sizeof(T), (size_t)rows * sizeof(T), (size_t)q));
        qil_ctx_free(ctx, tmp);
        return QIL_OK;
    };
    if (tall && q >= 17) {
        void* nb_ = nullptr;
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)q * sizeof(double), &nb_));
        QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)q), dim3(256), 0, (const T*)B, ldb, p, (double*)nb_)));
        std::vector<double> cn((size_t)q);
        QIL_TRY(qil_read_back(ctx, cn.data(), nb_, (size_t)q * sizeof(double)));
        qil_ctx_free(ctx, nb_);
        bool finite = true;
        for (double v : cn) finite = finite && std::isfinite(v);
        std::vector<int> perm((size_t)q);
        std::iota(perm.begin(), perm.end(), 0);
        if (finite) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return cn[(size_t)a] > cn[(size_t)b]; });
        bool ident = true;
        for (long long j = 0; j < q; ++j) ident = ident && perm[(size_t)j] == (int)j;
        // only GRADED operands gain (column norms over more than three decades: every site of a truncating sweep over a product);
        // on flat ones -- compress! of a random state: ratios of 1.2 ... 10 -- the order does not change the sweep count and the
        // permutation would only cost (measured, c64 chi 256 -> 128: 96 sweeps either way, 55 -> 62 ms with it)
        static const double sort_grade = 1e3;
        if (!finite || !(cn[(size_t)perm[0]] > sort_grade * cn[(size_t)perm[(size_t)q - 1]])) ident = true;
        // how far from sorted the columns are: mean displacement / (q / 3) (1 = a random order, 0 = sorted)
        double disorder = 0.0;
        for (long long j = 0; j < q; ++j) disorder += std::fabs((double)perm[(size_t)j] - (double)j);
        disorder /= std::max(1.0, (double)q * (double)q / 3.0);
        // ... and only columns that are OUT OF ORDER gain: the sites of compress!'s later passes and of the fused route arrive as
        // A (U S), nearly sorted (disorder 0.00 ... 0.11 measured): sorting them changed no sweep count (exact route 509 vs 506
        // sweeps) and cost 2-3 % (8 small launches per SVD); the sites of a product's truncating sweep come in bond order, 0.38 ... 0.68
        static const double sort_disorder = 0.2;
        if (disorder < sort_disorder) ident = true;
        if (dbg) fprintf(stderr, "[svd-left] %lld x %lld: column norms %.3g ... %.3g, disorder %.3f%s\n", p, q, finite ? cn[(size_t)perm[0]] : 0.0,
                         finite ? cn[(size_t)perm[(size_t)q - 1]] : 0.0, disorder, ident ? " (left as they are)" : "");
        if (!ident) {
            std::vector<int> both((size_t)(2 * q));
            for (long long j = 0; j < q; ++j) {
                both[(size_t)j] = perm[(size_t)j];
                both[(size_t)(q + perm[(size_t)j])] = (int)j;
            }
            void *hp = nullptr, *dp = nullptr, *tmp = nullptr;
            int slot = -1;
            const size_t up = both.size() * sizeof(int);
            QIL_TRY(qil_ctx_alloc(ctx, up, &permbuf));
            QIL_TRY(qil_stage_acquire(ctx, up, &hp, &dp, &slot));
            memcpy(hp, both.data(), up);
            QIL_TRY(qil_stage_push(ctx, slot, up));
            QIL_TRY(qil_dev_copy(ctx, permbuf, dp, up));
            qil_stage_commit(ctx, slot);
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(p * q) * sizeof(T), &tmp));
            const unsigned g = (unsigned)std::min<long long>((p * q + 1023) / 1024, 4096);
            QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3(g), dim3(1024), 0, (const T*)B, ldb, p, static_cast<const int*>(permbuf),
                                                      (const double*)nullptr, static_cast<T*>(tmp), p, (int)q, 0)));
            QIL_TRY(qil_dev_copy2d(ctx, B, (size_t)ldb * sizeof(T), tmp, (size_t)p * sizeof(T), (size_t)p * sizeof(T), (size_t)q));
            qil_ctx_free(ctx, tmp);
            permuted = true;
            if (dbg) fprintf(stderr, "[svd-left] %lld x %lld: columns sorted by norm (%.3g ... %.3g)\n", p, q, cn[(size_t)perm[0]], cn[(size_t)perm[(size_t)q - 1]]);
        }
    }
    if (tall) {
        bool known = false;
        QIL_TRY(qr_impl<T>(ctx, p, q, B, ldb, R, k, &known, cert_cutoff > 0.0 ? &rinv : nullptr));
        bool ok = true;
        QIL_TRY(qr_reorthogonalise<T>(ctx, p, q, B, ldb, R, k, known, &rinv, dbg, &ok));
        if (!ok) {                                   // B = Q R reproduces the operand: hand it back intact
            void* tmp = nullptr;
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(p * q) * sizeof(T), &tmp));
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, p, q, q, B, ldb, R, k, static_cast<T*>(tmp), p));
            QIL_TRY(qil_dev_copy2d(ctx, B, (size_t)ldb * sizeof(T), tmp, (size_t)p * sizeof(T), (size_t)p * sizeof(T), (size_t)q));
            qil_ctx_free(ctx, tmp);
            QIL_TRY(put_back_columns(B, ldb, p));
            release();
            return QIL_OK;
        }
        Qm = B;
        ldq = ldb;
        qrows = p;
        // Which triangular factor to rotate.  On a GRADED operand (singular values over several decades: the first
        // truncating SVD of a sweep, whose site carries the whole untruncated Schmidt spectrum of its bond; products before
        // truncation) one-sided Jacobi on the columns of R crawls -- 24-40 sweeps against 11-12 on the rows, i.e. on the
        // columns of the lower-triangular factor of a second QR (Drmac-Veselic; numpy: 256 columns, 6 / 12 decades; measured
        // here: the first 256-column SVD of compress! chi 256 -> 128 took 35 sweeps, the later, truncated ones 13).  On flat
        // spectra the two orientations need the same sweeps and the second QR (~0.8 ms at 256 columns) is not worth it.  The
        // grading shows in R's diagonal: mean |r_ii|^2 against min |r_ii|^2 (measured on the truncated sites of the same
        // sweep, ratio ~1e5: 13 sweeps on R, 9 after the second QR).
        bool qr2 = false;
        qil_progress_phase(ctx, 2);
        static const double grade = 1e3;   // (0 = never; 1e3: compress! chi 256 -> 128 85.8 -> 73.4 ms, 512 -> 256 211 -> 197 ms, complex 112 -> 104 ms, exact compress!(apply) 389 -> 348 ms; 1e5 / 1e8: 77 / 75 ms)
        if (!qr2 && grade > 0.0) {
            void* st = nullptr;
            constexpr int NB = 16;
            QIL_TRY(qil_ctx_alloc(ctx, 2 * NB * sizeof(double), &st));
            double hb[2 * NB];
            QIL_TRY((qil_klaunch<tri_stats_k<T>>(ctx, dim3(NB), dim3(256), 0, (const T*)R, k, (int)k, 1, (double*)st)));
            QIL_TRY(qil_read_back(ctx, hb, st, sizeof(hb)));
            qil_ctx_free(ctx, st);
            double fro2 = 0, dmin = 1e300;
            for (int bI = 0; bI < NB; ++bI) {
                fro2 += hb[2 * bI];
                dmin = std::min(dmin, hb[2 * bI + 1]);
            }
            // ... but not a numerically rank-deficient one (every product bond before its truncation: min |r_ii| at rounding
            // level): its null directions are set aside by the negligible-column rule, nothing crawls, and the second QR of
            // a deficient factor only costs (zT MPO final compression 137 -> 167 ms with it)
            static const double grade_max = 1e24;
            qr2 = std::isfinite(fro2) && fro2 > grade * (double)k * dmin && fro2 < grade_max * (double)k * dmin;
            if (dbg) fprintf(stderr, "[svd-left] %lld x %lld: mean / min |r_ii|^2 = %.3g -> %s\n", p, q, fro2 / ((double)k * std::max(dmin, 1e-300)), qr2 ? "second QR" : "rotate R");
            // A numerically RANK-DEFICIENT factor that is about to be truncated by a cutoff (product bonds before their
            // truncation): rotating the k columns of R crawls (14-18 sweeps at 128 columns: the null space is a k - r fold
            // degenerate cluster), and most of the work is spent on directions the cutoff discards.  The rows of R say which:
            // dropping the rows with the smallest norms changes A by EXACTLY their weight (A = Q R), so rows are dropped while
            // their weight stays below `deflate` (1e-6 of the caller's cutoff) of the total, and the one-factor SVD of
            // the remaining r x k block -- a wide, full-rank operand: QR of its r columns, r x r rotations -- gives the same
            // factors: U = Q[:, K] U_K, S V^H = S_K V_K^H.
            const bool deficient = std::isfinite(fro2) && fro2 >= grade_max * (double)k * dmin;
            if (deficient && deflate > 0.0 && k >= 64) {                         // (such a factor never passes the certificate: min |r_ii| settles it)
                int done = 0;
                QIL_TRY((svd_left_deflated<T>(ctx, p, k, Qm, ldq, R, X, Uiso, ldu, S_host, SVh, ldsvh, negl_rel, deflate, dbg, &done)));
                if (done) {
                    QIL_TRY(put_back_columns(SVh, ldsvh, k));
                    lap("deflated route");
                    release();
                    *handled = 1;
                    return QIL_OK;
                }
            }
        }
        if (qr2) {
            // R^H = Q1 R1; the columns of X = R1^H are rotated (R = X Q1^H has the same left singular vectors)
            void* r1 = nullptr;
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * k) * sizeof(T), &r1));
            QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3(gk), dim3(256), 0, (const T*)R, k, k, k, X, k)));
            bool known1 = false;
            QIL_TRY(qr_impl<T>(ctx, k, k, X, k, static_cast<T*>(r1), k, &known1));
            QIL_TRY(qr_reorthogonalise<T>(ctx, k, k, X, k, static_cast<T*>(r1), k, known1, &rinv, dbg, nullptr));
            QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3(gk), dim3(256), 0, (const T*)r1, k, k, k, X, k)));
            qil_ctx_free(ctx, r1);
        } else {
            QIL_TRY(qil_dev_copy(ctx, X, R, (size_t)(k * k) * sizeof(T)));
        }
    } else {
        // B^H = Q R  =>  B = R^H Q^H: the left singular vectors of B are those of X = R^H
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(q * p) * sizeof(T), &bh));
        QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3((unsigned)std::min<long long>((p * q + 255) / 256, 65536)), dim3(256), 0, (const T*)B, ldb, p, q, static_cast<T*>(bh), q)));
        bool known = false;
        QIL_TRY(qr_impl<T>(ctx, q, p, static_cast<T*>(bh), q, R, k, &known));
        bool ok = true;
        QIL_TRY(qr_reorthogonalise<T>(ctx, q, p, static_cast<T*>(bh), q, R, k, known, nullptr, dbg, &ok));
        if (!ok) {
            release();
            return QIL_OK;
        }
        QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3(gk), dim3(256), 0, (const T*)R, k, k, k, X, k)));
        if (deflate > 0.0 && k >= 64) {                          // rank-deficient products: the negligible rows of R leave the problem
            int done = 0;
            QIL_TRY((svd_left_deflated_wide<T>(ctx, k, q, static_cast<const T*>(bh), q, X, Uiso, ldu, S_host, SVh, ldsvh, negl_rel, deflate, dbg, &done)));
            if (done) {
                lap("deflated route (wide)");
                release();
                *handled = 1;
                return QIL_OK;
            }
        }
    }
    lap("QR");
    qil_progress_phase(ctx, 3);
    if (cert_cutoff > 0.0) {
        // the caller truncates by cutoff only and does not read the singular values: if nothing can be dropped, the thin
        // QR is the gauge step (*handled = 2, S_host untouched)
        bool certified = false;
        QIL_TRY(certify_no_truncation<T>(ctx, R, k, (int)k, cert_cutoff, std::exchange(rinv, nullptr), &certified));   // (it frees R^-1)
        if (certified) {
            if (tall) {                                  // B = Q R: Uiso = Q (in B), S V^H = R
                QIL_TRY(qil_dev_copy2d(ctx, Uiso, (size_t)ldu * sizeof(T), Qm, (size_t)ldq * sizeof(T), (size_t)p * sizeof(T), (size_t)k));
                QIL_TRY(qil_dev_copy2d(ctx, SVh, (size_t)ldsvh * sizeof(T), R, (size_t)k * sizeof(T), (size_t)k * sizeof(T), (size_t)q));
                QIL_TRY(put_back_columns(SVh, ldsvh, k));
            } else {                                     // p < q: the whole row space is kept: Uiso = I, S V^H = B
                QIL_TRY(qil_dev_zero2d(ctx, Uiso, (size_t)ldu * sizeof(T), (size_t)k * sizeof(T), (size_t)k));
                QIL_TRY((qil_klaunch<set_identity_k<T>>(ctx, dim3(gk), dim3(256), 0, Uiso, ldu, (int)k)));
                QIL_TRY(qil_dev_copy2d(ctx, SVh, (size_t)ldsvh * sizeof(T), B, (size_t)ldb * sizeof(T), (size_t)p * sizeof(T), (size_t)q));
            }
            QIL_HIP(hipGetLastError());
            lap("certificate: QR gauge");
            release();
            *handled = 2;
            return QIL_OK;
        }
        lap("certificate: declined");
    }
    qil_progress_phase(ctx, 4);
    QIL_TRY(qil_ctx_alloc(ctx, 512, &flag));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)k * sizeof(double), &nrm));
    if (negl_rel > 0.0) {
        QIL_TRY(qil_ctx_alloc(ctx, 256, &negl));
        QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)k), dim3(256), 0, (const T*)X, k, k, (double*)nrm)));
        QIL_TRY((qil_klaunch<negligible_threshold_k>(ctx, dim3(1), dim3(256), 0, (const double*)nrm, (int)k, negl_rel, (double*)negl)));
    }
    const double tol = std::max(1e-15, 4.0 * 1.1e-16 * std::sqrt((double)k));
    const int nblk = (int)(((k + bb - 1) / bb + 1) / 2 * 2);
    int sweeps = 0;
    // the rounds of one sweep
    auto launch_rounds = [&](int* fl, const int* prev) -> int {
        for (int round = 0; round < nblk - 1; ++round) {
#define QIL_NOV(BBv, KMv, Gv) QIL_TRY((launch_block_round_nov<T, BBv, KMv, Gv>(ctx, X, k, (int)k, nblk, round, tol, fl, (const double*)negl, prev)))
            {
                switch (km) {
                    case 1: QIL_NOV(8, 1, 64); break;
                    case 2: QIL_NOV(8, 2, 64); break;
                    case 3: QIL_NOV(8, 3, 64); break;
                    case 4: QIL_NOV(8, 4, 64); break;
                    case 5: QIL_NOV(8, 5, 64); break;
                    case 6: QIL_NOV(8, 6, 64); break;
                    case 7: QIL_NOV(8, 7, 64); break;
                    case 8: QIL_NOV(8, 8, 64); break;
                    case 9: QIL_NOV(8, 9, 64); break;
                    default:
                        if constexpr (sizeof(T) == 8) QIL_NOV(8, 10, 64);
                        break;
                }
            }
#undef QIL_NOV
        }
        return QIL_OK;
    };
    bool gram_done = false;
    // (r05 built the persistent form -- every round of every sweep of one SVD in ONE launch of nblk / 2 co-resident workgroups, a
    // device-scope barrier between rounds, the convergence decision on the device -- and measured it against these per-round
    // launches: chi 256 -> 128 45.0 -> 43.6 ms, chi 512 -> 256 110.7 -> 119.1 ms, exact compress!(apply) 281 -> 272 ms with the kernel
    // time of its complex rounds UP 19 %: a barrier through L2 costs what a dispatch costs.  Removed again, VERDICT r04 item 3's
    // stop rule; code in commit 674496a, evidence profiles/r05_persist_{compare,trace}.txt.)
    if constexpr (sizeof(T) == 8) if (gbb) {                     // (no complex instantiation of the Gram-round kernels: r05)
        gram_done = true;
        // Gram-matrix block rounds on the matrix cores.  The host stays ONE SWEEP AHEAD of its read-backs: sweep s + 1 is
        // enqueued before the flags of sweep s have come back, each of its launches first looks at those flags on the device
        // and does nothing if sweep s had already converged -- the stream never waits for a host round trip.
        constexpr int MAXS = 40;
        int* dflag = static_cast<int*>(flag);                    // [MAXS][2]
        QIL_TRY(qil_dev_zero(ctx, dflag, (size_t)2 * MAXS * sizeof(int)));
        uint64_t ticket[2] = {0, 0};
        auto enqueue = [&](int sw) -> int {
            for (int round = 0; round < nblk - 1; ++round) {
                const int* prev = sw > 0 ? dflag + 2 * (sw - 1) : nullptr;
                if (gbb == 16)
                    QIL_TRY((launch_gram_round<T, 16>(ctx, X, k, (int)k, nblk, round, tol, dflag + 2 * sw, prev, (const double*)negl)));
                else
                    QIL_TRY((launch_gram_round<T, 8>(ctx, X, k, (int)k, nblk, round, tol, dflag + 2 * sw, prev, (const double*)negl)));
            }
            return qil_read_back_post(ctx, dflag + 2 * sw, 2 * sizeof(int), &ticket[sw & 1]);
        };
        int st = enqueue(0);
        for (; st == QIL_OK && sweeps < MAXS; ++sweeps) {
            if (sweeps + 1 < MAXS) st = enqueue(sweeps + 1);
            if (st != QIL_OK) break;
            int hv[2] = {0, 0};
            st = qil_read_back_wait(ctx, ticket[sweeps & 1], hv, sizeof(hv));
            if (st != QIL_OK) break;
            if (dbg) fprintf(stderr, "[svd-left] gram sweep %d (%lld cols, blocks of %d): rotated=%d above-quadratic=%d\n", sweeps, k, bb, hv[0], hv[1]);
            if (!hv[1]) break;
        }
        QIL_TRY(st);
    }
    if (!gram_done) {
        // vector rounds (complex operands, f64 ones too tall for the Gram workspace): the host stays one sweep ahead of its
        // read-backs here too (r05: until then every sweep ended in a host round trip, ~8 per SVD -- the persistent-kernel
        // experiment's only gain on the exact route was their absence)
        constexpr int MAXS = 40;
        int* dflag = static_cast<int*>(flag);                    // [MAXS][2]
        QIL_TRY(qil_dev_zero(ctx, dflag, (size_t)2 * MAXS * sizeof(int)));
        uint64_t ticket[2] = {0, 0};
        auto enqueue = [&](int sw) -> int {
            QIL_TRY(launch_rounds(dflag + 2 * sw, sw > 0 ? dflag + 2 * (sw - 1) : nullptr));
            return qil_read_back_post(ctx, dflag + 2 * sw, 2 * sizeof(int), &ticket[sw & 1]);
        };
        int st = enqueue(0);
        for (; st == QIL_OK && sweeps < MAXS; ++sweeps) {
            if (sweeps + 1 < MAXS) st = enqueue(sweeps + 1);
            if (st != QIL_OK) break;
            int hv[2] = {0, 0};
            st = qil_read_back_wait(ctx, ticket[sweeps & 1], hv, sizeof(hv));
            if (st != QIL_OK) break;
            if (dbg) fprintf(stderr, "[svd-left] sweep %d (%lld cols, blocks of %d): rotated=%d above-quadratic=%d\n", sweeps, k, bb, hv[0], hv[1]);
            if (!hv[1]) break;
        }
        QIL_TRY(st);
    }
    lap("sweeps");
    qil_progress_phase(ctx, 5);
    QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)k), dim3(256), 0, (const T*)X, k, k, (double*)nrm)));
    std::vector<double> sig((size_t)k);
    QIL_TRY(qil_read_back(ctx, sig.data(), nrm, (size_t)k * sizeof(double)));
    std::vector<int> perm((size_t)k);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return sig[(size_t)a] > sig[(size_t)b]; });
    std::vector<double> inv((size_t)k);
    for (long long j = 0; j < k; ++j) {
        const double sv = sig[(size_t)perm[(size_t)j]];
        S_host[j] = sv;
        inv[(size_t)j] = sv > 0 ? 1.0 / sv : 0.0;
    }
    void *hp = nullptr, *dp = nullptr;
    int slot = -1;
    const size_t up = (size_t)k * (sizeof(double) + sizeof(int));
    QIL_TRY(qil_stage_acquire(ctx, up, &hp, &dp, &slot));
    memcpy(hp, inv.data(), (size_t)k * sizeof(double));
    memcpy(static_cast<char*>(hp) + (size_t)k * sizeof(double), perm.data(), (size_t)k * sizeof(int));
    QIL_TRY(qil_stage_push(ctx, slot, up));
    const double* scd = static_cast<const double*>(dp);
    const int* permd = reinterpret_cast<const int*>(static_cast<const char*>(dp) + (size_t)k * sizeof(double));
    // W = normalised rotated columns in sorted order
    T* Wm = nullptr;
    long long ldw = k;
    if (tall) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * k) * sizeof(T), &wbuf));
        Wm = static_cast<T*>(wbuf);
    } else {
        Wm = Uiso;
        ldw = ldu;
    }
    QIL_TRY((qil_klaunch<gather_cols_k<T>>(ctx, dim3(gk), dim3(256), 0, (const T*)X, k, k, permd, scd, Wm, ldw, (int)k, 0)));
    qil_stage_commit(ctx, slot);
    if (tall) {
        QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, qrows, k, k, Qm, ldq, Wm, ldw, Uiso, ldu));          // Uiso = Q W
        QIL_TRY(gemm_dispatch<T>(ctx, cj, 0, k, q, k, Wm, ldw, R, k, SVh, ldsvh));               // S V^H = W^H R
        QIL_TRY(put_back_columns(SVh, ldsvh, k));
    } else {
        QIL_TRY(gemm_dispatch<T>(ctx, cj, 0, k, q, p, Wm, ldw, B, ldb, SVh, ldsvh));             // S V^H = W^H B
    }
    QIL_HIP(hipGetLastError());
    lap("factors out");
    release();
    *handled = 1;
    return QIL_OK;
}

// Thin SVD A = U diag(S) Vh by one-sided Jacobi on the SHORT side.
//   1. orientation: the work matrix has rows >= cols (A^H if m < n);
//   2. tall-skinny (rows >= 8 cols): QR first, Jacobi on the cols x cols factor R, U = Q U_R;
//   3. three regimes by column count: <= 96 columns with (at least) A resident in LDS -- the whole iteration is one
//      launch of one workgroup (jacobi_fused); >= 640 columns -- QR, then GEMM-shaped block Jacobi sweeps on R^H
//      (block_jacobi); in between QR, then in-LDS block rounds on R^H (jacobi_block_round); one launch per scalar
//      tournament round (jacobi_round) remains for operands too tall for LDS and as the fallback of the block path.
template <class T>
int svd_impl(qil_context* ctx, long long m, long long n, T* A, long long lda, T* U, long long ldu,
             double* S_host, T* Vh, long long ldvh, double negl_rel) {
    const long long r0 = std::min(m, n);
    if (r0 == 0) return QIL_OK;
    const bool dbg = getenv("QIL_SVD_DEBUG") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        (void)qil_stream_sync(ctx);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[svd] %lld x %lld: %s %.1f ms\n", m, n, what,
                std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    const bool flip = m < n;
    T* Wk = A;           // work matrix (rows x cols), columns get orthogonalised
    long long ldw = lda, rows = m, cols = n;
    void* tbuf = nullptr;
    if (flip) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(m * n) * sizeof(T), &tbuf));
        Wk = static_cast<T*>(tbuf);
        ldw = n;
        rows = n;
        cols = m;
        QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3((unsigned)std::min<long long>((m * n + 255) / 256, 65536)), dim3(256), 0, A, lda, m, n, Wk, ldw)));
    }
    // tall-skinny: Wk = Q R, rotate R instead.  Large column counts (block path): always, and rotate R^H --
    // the rows of a triangular factor are far closer to orthogonal than its columns, which saves sweeps
    // (the classical preconditioning of one-sided Jacobi); then R^H = L S V^H gives Wk = (Q V) S L^H.
    static const long long bj_min = 640;   // (crossover with the in-LDS block rounds: 600-700 columns)
    // mid-size operands too: neutral on random matrices, but graded / low-rank spectra -- what truncation sees after an
    // apply -- need 2-4x fewer sweeps (512 x 256 graded: 36 -> 9 ms including the QR)
    static const long long rt_min = 97;
    const bool blocked = cols >= bj_min;
    bool rt = cols >= rt_min;   // (blocked implies it)
    T* Q = nullptr;
    long long ldq = 0, qrows = 0;
    void *rbuf = nullptr, *rtbuf = nullptr, *abuf = nullptr;
    static const long long qr_ratio = 8;
    if ((rows >= qr_ratio * cols && rows >= 512) || rt) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(cols * cols) * sizeof(T), &rbuf));
        bool known = false;
        QIL_TRY(qr_impl<T>(ctx, rows, cols, Wk, ldw, static_cast<T*>(rbuf), cols, &known));
        bool q_ok = true;
        QIL_TRY(qr_reorthogonalise<T>(ctx, rows, cols, Wk, ldw, static_cast<T*>(rbuf), cols, known, nullptr, dbg, &q_ok));
        if (!q_ok) {
            // the re-factorisations did not reach an orthonormal basis (spectra graded to rounding level on very tall
            // operands): Q R still reproduces the operand to rounding, so it is rebuilt and rotated as it is --
            // slower (rows stay long), but one-sided Jacobi needs no conditioning assumption
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(rows * cols) * sizeof(T), &abuf));
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, rows, cols, cols, Wk, ldw, static_cast<const T*>(rbuf), cols,
                                     static_cast<T*>(abuf), rows));
            Wk = static_cast<T*>(abuf);
            ldw = rows;
            qil_ctx_free(ctx, rbuf);
            rbuf = nullptr;
            rt = false;
        } else {
            Q = Wk;
            ldq = ldw;
            qrows = rows;
            Wk = static_cast<T*>(rbuf);
            ldw = cols;
            rows = cols;
        }
        if (rt) {
            QIL_TRY(qil_ctx_alloc(ctx, (size_t)(cols * cols) * sizeof(T), &rtbuf));
            QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3((unsigned)std::min<long long>((cols * cols + 255) / 256, 65536)), dim3(256), 0, (const T*)Wk, ldw, cols, cols, static_cast<T*>(rtbuf), cols)));
            Wk = static_cast<T*>(rtbuf);
        }
    }
    lap("orientation + QR");
    void *vbuf = nullptr, *flag = nullptr, *nrm = nullptr, *permd = nullptr, *scd = nullptr, *xbuf = nullptr;
    void* negl = nullptr;         // device scalar: squared norm below which a column is rounding residue (or null)
    if (!blocked) QIL_TRY(qil_ctx_alloc(ctx, (size_t)(cols * cols) * sizeof(T), &vbuf));
    QIL_TRY(qil_ctx_alloc(ctx, 256, &flag));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)2 * (cols + BJ_W) * sizeof(double), &nrm));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)cols * sizeof(int), &permd));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)cols * sizeof(double), &scd));
    T* V = static_cast<T*>(vbuf);
    long long ldv = cols;
    long long nj = cols;          // columns of the rotated work area (> cols only with block padding)
    const int ncol = (int)cols;
    // convergence threshold on |a_p . a_q| / (|a_p| |a_q|): 1e-15, but never below the rounding noise of the
    // dot products themselves (~ eps sqrt(rows)), which long columns cannot get under
    const double tol = std::max(1e-15, 4.0 * 1.1e-16 * std::sqrt((double)rows));
    const size_t lds_a = (size_t)((rows | 1) * cols) * sizeof(T);
    const size_t lds_av = lds_a + (size_t)((cols | 1) * cols) * sizeof(T);
    // one workgroup for the whole iteration only while (at least) A lives in LDS; a single workgroup working out of
    // L2 is slower than the tournament launches, which spread the pairs over the chip
    if (ncol <= 96 && rows * cols <= (1LL << 19) &&
        (lds_av <= 150 * 1024 || (rows <= 128 && lds_a <= 150 * 1024))) {
        if (lds_av <= 150 * 1024) {
            QIL_TRY((qil_klaunch<jacobi_fused_k<T, 1>>(ctx, dim3(1), dim3(1024), lds_av, Wk, ldw, (int)rows, V, cols, ncol, tol, 40, (double*)nrm, negl_rel)));
        } else {   // A only; one DPP row per pair only up to 128 rows
            QIL_TRY((qil_klaunch<jacobi_fused_k<T, 2>>(ctx, dim3(1), dim3(1024), lds_a, Wk, ldw, (int)rows, V, cols, ncol, tol, 40, (double*)nrm, negl_rel)));
        }
    } else {
        bool bj_done = false;
        if (negl_rel > 0.0) {
            QIL_TRY(qil_ctx_alloc(ctx, 256, &negl));
            QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)cols), dim3(256), 0, (const T*)Wk, ldw, rows, (double*)nrm)));
            QIL_TRY((qil_klaunch<negligible_threshold_k>(ctx, dim3(1), dim3(256), 0, (const double*)nrm, (int)cols, negl_rel, (double*)negl)));
        }
        if (blocked) {
            // GEMM-shaped block sweeps; the scalar tournament below only runs if they hit their sweep limit
            long long ldx = 0, cpad = 0;
            QIL_TRY(block_jacobi<T>(ctx, rows, cols, Wk, ldw, tol, 20, &xbuf, &ldx, &cpad, &bj_done,
                                    (const double*)negl));
            Wk = static_cast<T*>(xbuf);
            ldw = ldx;
            V = Wk + rows;
            ldv = ldx;
            nj = cpad;
            lap("block sweeps");
        } else {
            QIL_TRY((qil_klaunch<set_identity_k<T>>(ctx, dim3((unsigned)std::min<long long>((cols * cols + 255) / 256, 65536)), dim3(256), 0, V, cols, (int)cols)));
        }
        const int nn = (int)nj, npad = nn + (nn & 1);
        // in-LDS block rounds when 2 BB columns of A and V fit one CU's LDS (not after the GEMM-shaped block sweeps:
        // their fallback keeps the scalar rounds)
        int bb = 0;
        if (!blocked && rows <= (1 << 20)) {
            const size_t per_col = (size_t)((rows | 1) + (cols | 1)) * sizeof(T);
            if (16 * per_col <= 150 * 1024) bb = 8;
            else if (8 * per_col <= 150 * 1024) bb = 4;
        }
        const int nblk = bb ? (int)(((cols + bb - 1) / bb + 1) / 2 * 2) : 0;
        for (int sweep = 0; sweep < 40 && nn > 1 && !bj_done; ++sweep) {
            QIL_TRY(qil_dev_zero(ctx, flag, 2 * sizeof(int)));
            if (bb) {
                const size_t lds = (size_t)2 * bb * ((rows | 1) + (cols | 1)) * sizeof(T);
                for (int round = 0; round < nblk - 1; ++round) {
                    if (bb == 8)
                        QIL_TRY((qil_klaunch<jacobi_block_round_k<T, 8>>(ctx, dim3(nblk / 2), dim3(512), lds, Wk, ldw, (int)rows, V, ldv, (int)cols, nn, nblk, round, round == 0 ? 1 : 0, tol, (int*)flag, (const double*)negl)));
                    else
                        QIL_TRY((qil_klaunch<jacobi_block_round_k<T, 4>>(ctx, dim3(nblk / 2), dim3(256), lds, Wk, ldw, (int)rows, V, ldv, (int)cols, nn, nblk, round, round == 0 ? 1 : 0, tol, (int*)flag, (const double*)negl)));
                }
            }
            for (int round = 0; round < npad - 1 && !bb; ++round)
                QIL_TRY((qil_klaunch<jacobi_round_k<T>>(ctx, dim3(npad / 2), dim3(256), 0, Wk, ldw, rows, V, ldv, (int)cols, nn, npad, round, tol, (int*)flag, (const double*)negl)));
            int hv[2] = {0, 0};
            QIL_TRY(qil_read_back(ctx, hv, flag, 2 * sizeof(int)));
            if (getenv("QIL_SVD_DEBUG")) fprintf(stderr, "[svd] scalar sweep %d (cols %lld): rotated=%d above-quadratic=%d\n", sweep, nj, hv[0], hv[1]);
            if (!hv[1]) break;   // nothing rotated, or only pairs already below the quadratic-phase level
        }
        QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)nj), dim3(256), 0, Wk, ldw, rows, (double*)nrm)));
        if (blocked)   // padding columns are zero in the V part too; genuine columns have unit V columns
            QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)nj), dim3(256), 0, (const T*)V, ldv, cols, (double*)nrm + nj)));
    }
    lap("scalar sweeps");
    std::vector<double> sig((size_t)nj * 2, 1.0);
    {
        const size_t down = (size_t)nj * (blocked && nj > 96 ? 2 : 1) * sizeof(double);
        QIL_TRY(qil_read_back(ctx, sig.data(), nrm, down));
    }
    std::vector<int> perm((size_t)nj);
    std::iota(perm.begin(), perm.end(), 0);
    const double* vn = sig.data() + nj;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) {
        const bool pa = vn[a] < 0.5, pb = vn[b] < 0.5;      // padding columns last
        if (pa != pb) return pb;
        return sig[(size_t)a] > sig[(size_t)b];
    });
    std::vector<double> inv((size_t)cols);
    for (long long j = 0; j < cols; ++j) {
        const double s = sig[(size_t)perm[(size_t)j]];
        S_host[j] = s;
        inv[(size_t)j] = s > 0 ? 1.0 / s : 0.0;
    }
    // permutation + reciprocal singular values go up through the context's event-guarded pinned ring when they fit a
    // slot: no stream synchronisation at the end of the call, so the device does not idle while the host enqueues
    // whatever follows (chains of small SVDs are bound by exactly that)
    const size_t up_bytes = (size_t)cols * (sizeof(double) + sizeof(int));
    int ring_slot = -1;
    if (up_bytes <= qil_context::kStSlotBytes) {
        void *hp = nullptr, *dp = nullptr;
        QIL_TRY(qil_stage_acquire(ctx, up_bytes, &hp, &dp, &ring_slot));
        memcpy(hp, inv.data(), (size_t)cols * sizeof(double));
        memcpy(static_cast<char*>(hp) + (size_t)cols * sizeof(double), perm.data(), (size_t)cols * sizeof(int));
        QIL_TRY(qil_stage_push(ctx, ring_slot, up_bytes));
        qil_ctx_free(ctx, scd);
        qil_ctx_free(ctx, permd);
        scd = dp;
        permd = static_cast<char*>(dp) + (size_t)cols * sizeof(double);
    } else {
        QIL_HIP(hipMemcpyAsync(permd, perm.data(), (size_t)cols * sizeof(int), hipMemcpyHostToDevice, qil_stream(ctx)));
        QIL_HIP(hipMemcpyAsync(scd, inv.data(), (size_t)cols * sizeof(double), hipMemcpyHostToDevice, qil_stream(ctx)));
    }
    // Work problem: Wk[:, perm] = Fw diag(S), Fw orthonormal columns, and Fv = V[:, perm]:  Wk = Fw S Fv^H.
    //   plain:        oriented A = Wk            = (Fw)   S (Fv)^H
    //   QR:           oriented A = Q Wk          = (Q Fw) S (Fv)^H
    //   QR, R^H:      oriented A = Q Wk^H        = (Q Fv) S (Fw)^H
    // and for the flipped orientation (A^H was factored) left and right swap once more.
    struct small_factor {
        const T* p;
        long long ld, nrows;
        const double* scale;
    };
    const small_factor fw{Wk, ldw, rows, (const double*)scd}, fv{V, ldv, cols, nullptr};
    const small_factor ls = rt ? fv : fw, rs = rt ? fw : fv;      // small left / right factors
    auto gather = [&](const small_factor& f, T* dst, long long ldd, int conjT) -> int {
        const unsigned g = (unsigned)std::min<long long>((f.nrows * cols + 255) / 256, 65536);
        return qil_klaunch<gather_cols_k<T>>(ctx, dim3(g), dim3(256), 0, f.p, f.ld, f.nrows, (const int*)permd, f.scale, dst, ldd, (int)cols, conjT);
    };
    void* lbuf = nullptr;
    const long long lrows = Q ? qrows : rows;
    if (Q) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(cols * cols) * sizeof(T), &lbuf));
        QIL_TRY(gather(ls, static_cast<T*>(lbuf), cols, 0));
    }
    if (!flip) {
        if (Q)
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, lrows, cols, cols, Q, ldq, static_cast<T*>(lbuf), cols, U, ldu));
        else
            QIL_TRY(gather(ls, U, ldu, 0));
        QIL_TRY(gather(rs, Vh, ldvh, 1));
    } else {
        QIL_TRY(gather(rs, U, ldu, 0));
        if (Q)   // Vh (cols x lrows) = (Q * small)^H = small^H * Q^H
            QIL_TRY(gemm_dispatch<T>(ctx, sizeof(T) == 16 ? 2 : 1, sizeof(T) == 16 ? 2 : 1, cols, lrows, cols,
                                     static_cast<T*>(lbuf), cols, Q, ldq, Vh, ldvh));
        else
            QIL_TRY(gather(ls, Vh, ldvh, 1));
    }
    QIL_HIP(hipGetLastError());
    if (ring_slot >= 0) {
        qil_stage_commit(ctx, ring_slot);
        scd = permd = nullptr;                                   // ring memory, not pool blocks
    } else {
        // perm/inv are host vectors read by async copies: finish before they go out of scope
        QIL_HIP(qil_stream_sync(ctx));
    }
    lap("factors out");
    if (tbuf) qil_ctx_free(ctx, tbuf);
    if (rbuf) qil_ctx_free(ctx, rbuf);
    if (rtbuf) qil_ctx_free(ctx, rtbuf);
    if (abuf) qil_ctx_free(ctx, abuf);
    if (lbuf) qil_ctx_free(ctx, lbuf);
    if (vbuf) qil_ctx_free(ctx, vbuf);
    if (xbuf) qil_ctx_free(ctx, xbuf);
    if (negl) qil_ctx_free(ctx, negl);
    qil_ctx_free(ctx, flag);
    qil_ctx_free(ctx, nrm);
    if (permd) qil_ctx_free(ctx, permd);
    if (scd) qil_ctx_free(ctx, scd);
    return QIL_OK;
}

// ------------------------------------------------------------------ Gram-Schmidt QR (CGS2), positive diagonal
// R[0:k, j0:j0+b] += C (k x b)
template <class T>
__device__ __forceinline__ void add_block_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ R, long long ldr, const T* __restrict__ C, long long ldc, int k,
                          int b) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < k * b; t += gridDim.x * blockDim.x) {
        const int i = t % k, j = t / k;
        R[i + ldr * j] = add_t(R[i + ldr * j], C[i + ldc * j]);
    }
}
template <class T>
struct add_block_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        add_block_body<T>(b, g, a...);
    }
};
// Column norms of a tall matrix: partial sums of squares per (chunk, column), then one small reduction.
template <class T>
__device__ __forceinline__ void col_sumsq_chunks_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ A, long long lda, long long m,
                                                        long long chunk_rows, double* __restrict__ part) {
    __shared__ double red[4];
    const long long r0 = blockIdx.y * chunk_rows, r1 = min(m, r0 + chunk_rows);
    const T* a = A + lda * blockIdx.x;
    double v[1] = {0};
    for (long long r = r0 + threadIdx.x; r < r1; r += 256) v[0] += abs2_t(a[r]);
    block_sum<1>(v, red);
    if (threadIdx.x == 0) part[blockIdx.y + (long long)gridDim.y * blockIdx.x] = v[0];
}
template <class T>
struct col_sumsq_chunks_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        col_sumsq_chunks_body<T>(b, g, a...);
    }
};
__device__ __forceinline__ void sqrt_sum_chunks_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ part, int nch,
                                                       double* __restrict__ out) {
    __shared__ double red[4];
    double v[1] = {0};
    for (int t = threadIdx.x; t < nch; t += 256) v[0] += part[t + (long long)nch * blockIdx.x];
    block_sum<1>(v, red);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt(v[0]);
}
struct sqrt_sum_chunks_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        sqrt_sum_chunks_body(b, g, a...);
    }
};
template <class T>
int col_norms_any(qil_context* ctx, const T* A, long long lda, long long m, long long n, double* out) {
    if (m < (1LL << 16)) {
        QIL_TRY((qil_klaunch<col_norms_k<T>>(ctx, dim3((unsigned)n), dim3(256), 0, A, lda, m, out)));
        QIL_HIP(hipGetLastError());
        return QIL_OK;
    }
    const long long chunk = std::max<long long>(4096, (m / 256 + 255) / 256 * 256);
    const int nch = (int)((m + chunk - 1) / chunk);
    void* part = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(nch * n) * sizeof(double), &part));
    QIL_TRY((qil_klaunch<col_sumsq_chunks_k<T>>(ctx, dim3((unsigned)n, (unsigned)nch), dim3(256), 0, A, lda, m, chunk, (double*)part)));
    QIL_TRY((qil_klaunch<sqrt_sum_chunks_k>(ctx, dim3((unsigned)n), dim3(256), 0, (const double*)part, nch, out)));
    QIL_HIP(hipGetLastError());
    qil_ctx_free(ctx, part);
    return QIL_OK;
}

// P[rows of chunk c, :] <- P[rows of chunk c, :] * Q2[c*b : (c+1)*b, :]   (second half of the tree: the
// chunk-local orthonormal factors times the factor of the stacked triangles)
template <class T, int B>
__device__ __forceinline__ void tsqr_apply_q2_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ P, long long lda, long long m, int b,
                                                     const T* __restrict__ Q2, long long ldq,
                                                     long long chunk_rows) {
    __shared__ T q2[B * B];
    const long long c = blockIdx.y;
    for (int t = threadIdx.x; t < B * B; t += 256) {
        const int i = t % B, j = t / B;
        q2[t] = (i < b && j < b) ? Q2[c * b + i + ldq * j] : T{};
    }
    __syncthreads();
    const long long r1 = min(m, (c + 1) * chunk_rows);
    for (long long r = c * chunk_rows + blockIdx.x * 256 + threadIdx.x; r < r1; r += (long long)gridDim.x * 256) {
        T in[B], out[B];
#pragma unroll
        for (int i = 0; i < B; ++i) in[i] = i < b ? P[r + lda * i] : T{};
#pragma unroll
        for (int j = 0; j < B; ++j) {
            T acc{};
#pragma unroll
            for (int i = 0; i < B; ++i) acc = fma_t(in[i], q2[i + B * j], acc);
            out[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < B; ++j)
            if (j < b) P[r + lda * j] = out[j];
    }
}
template <class T, int B>
struct tsqr_apply_q2_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        tsqr_apply_q2_body<T, B>(b, g, a...);
    }
};

// Tall-skinny QR of an m x b panel (b <= 16): a two-level tree.  ~512 workgroups orthonormalise their own
// row chunks (CGS2, same dependence rule, measured against the GLOBAL column norms so a chunk never
// normalises what is noise for the whole column), one workgroup factors the stacked triangles, and the
// chunk factors are multiplied by their b x b piece of that second factor.  Three launches that stream
// the panel with the whole chip instead of one CU.
template <class T>
int tsqr_panel(qil_context* ctx, long long m, int b, T* P, long long lda, T* R, long long ldr,
               const double* ref_norm) {
    const long long chunk = tsqr_chunk_rows(m);
    const long long nch = (m + chunk - 1) / chunk;
    void *rs = nullptr, *r2 = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(nch * b * b) * sizeof(T), &rs));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(b * b) * sizeof(T), &r2));
    T* Rs = static_cast<T*>(rs);
    QIL_TRY(gs_fused_launch<T>(ctx, (unsigned)nch, P, lda, m, b, Rs, nch * b, ref_norm, chunk));
    QIL_TRY(gs_fused_launch<T>(ctx, 1u, Rs, nch * b, nch * b, b, static_cast<T*>(r2), (long long)b, ref_norm, 0LL));
    QIL_TRY((qil_klaunch<tsqr_apply_q2_k<T, 16>>(ctx, dim3((unsigned)std::min<long long>((chunk + 255) / 256, 64), (unsigned)nch), dim3(256), 0, P, lda, m, b, (const T*)Rs, nch * b, chunk)));
    QIL_HIP(hipGetLastError());
    if (R)
        QIL_TRY(qil_dev_copy2d(ctx, R, (size_t)ldr * sizeof(T), r2, (size_t)b * sizeof(T), (size_t)b * sizeof(T),
                                 (size_t)b));
    qil_ctx_free(ctx, rs);
    qil_ctx_free(ctx, r2);
    return QIL_OK;
}

// Which kernels factor an m x n operand: every size rule of the thin QR in one place.  qr_impl below switches on the struct this
// fills and qil_qr_plan hands it to the tests.  cx: complex elements.
void qr_plan(bool cx, long long m, long long n, qil_qr_plan_info* p) {
    static const long long TALL = 2048;
    const size_t esz = cx ? 16 : 8;
    *p = qil_qr_plan_info{};
    // Cholesky QR first where it pays (from a few panels on) and while it keeps succeeding on this context: a numerically
    // rank-deficient operand (product bonds, deficient sketches) costs the attempt a Gram product, a partial factorisation and
    // one synchronisation, so after a refusal the next attempts are skipped
    // (r05: skinny tall panels up to 2^24 entries too -- the 32768 x 133 sketch bases of the n = 30 encoder's root split sat just
    // above 2^22 and took the Householder tree at 2.2 ms each, five per split)
    p->cholesky_eligible = n >= 64 && n <= 1024 && m >= n && (m * n <= (1LL << 22) || (n <= 256 && m * n <= (1LL << 24)));
    // one launch for the whole factorisation: single panels, and anything whose slice fits one CU's LDS
    const bool fits_lds = gs_fused_lds_bytes(esz, m, n) <= QR_LDS_BUDGET;
    // panels go through the row-chunk tree from TALL rows on, and already from 640 rows when a rows x 16 panel does
    // not fit LDS (complex panels above ~580 rows): its 512-row chunks do, and a single workgroup factoring such a
    // panel out of L2 takes ~220-290 us instead of three short launches
    const bool panel16_fits = gs_fused_lds_bytes(esz, m, 16) <= QR_LDS_BUDGET;
    static const long long tree_min = 640;        // (1024 -> 600: exact compress! of the bond-1008 product 476 -> 455 ms, neutral elsewhere)
    const bool tree = m >= TALL || (!panel16_fits && m >= tree_min);
    // up to `fused_max` columns the CGS2 kernel does the whole factorisation in one launch; beyond, whenever a Householder
    // panel fits, one panel launch (n <= 32) or the blocked route below is faster even where the operand fits one CU's LDS
    // (128 x 64: 274 -> ~140 us -- the CGS2 kernel pays ~4 us per column, the Householder panel ~1.5; compress! chi 64 -> 32
    // 28 -> 24.5 ms, 128 -> 64 50 -> 42 ms; narrower panels measured equal within noise either way)
    static const long long fused_max = 16;
    const bool hh_ok = !tree && n > fused_max && hh_panel_fits_sized(esz, m, (int)std::min<long long>(n, 32));
    // the kernel of one m x b panel, and what its launcher will derive from (m, b)
    bool cgs2_all_lds = true;
    auto panel = [&](int b) -> int {
        if (tree && b <= 16) {
            p->has_tree = 1;
            p->tree_chunk = tsqr_chunk_rows(m);
            p->tree_chunks = (m + p->tree_chunk - 1) / p->tree_chunk;
            p->tree_last_rows = m - (p->tree_chunks - 1) * p->tree_chunk;
            return QIL_QR_PANEL_TREE;
        }
        if (p->route != QIL_QR_SINGLE_CGS2 && hh_panel_fits_sized(esz, m, b)) {
            p->has_hh = 1;
            p->hh_km = hh_panel_km(m);
            p->hh_waves = cx ? hh_panel_waves_of<c64>(p->hh_km) : hh_panel_waves_of<double>(p->hh_km);
            return QIL_QR_PANEL_HH;
        }
        if (gs_fused_lds_bytes(esz, m, b) <= QR_LDS_BUDGET) {
            p->has_cgs2_lds = 1;
            return QIL_QR_PANEL_CGS2_LDS;
        }
        p->has_cgs2_global = 1;
        cgs2_all_lds = false;
        return QIL_QR_PANEL_CGS2_GLOBAL;
    };
    if (hh_ok && n <= 32) {
        p->route = QIL_QR_SINGLE_HH;
    } else if (n <= 16 || (fits_lds && !hh_ok)) {
        p->route = tree && n <= 16 ? QIL_QR_SINGLE_TREE : QIL_QR_SINGLE_CGS2;
    } else {
        p->route = QIL_QR_BLOCKED;
    }
    if (p->route != QIL_QR_BLOCKED) {
        p->panel_width = p->last_panel_width = (int)n;
        p->panel_kind = p->last_panel_kind = panel((int)n);
    } else {
        // panel width: 32 columns while a rows x 32 panel still fits one CU's LDS (half the launches), else 16
        const bool wide = !tree && gs_fused_lds_bytes(esz, m, 32) <= QR_LDS_BUDGET;
        p->panel_width = wide ? 32 : 16;
        p->last_panel_width = (int)(n - (n - 1) / p->panel_width * p->panel_width);
        p->panel_kind = panel(p->panel_width);
        p->last_panel_kind = panel(p->last_panel_width);
    }
    p->fused_in_lds = p->has_cgs2_lds && cgs2_all_lds;
    p->fused_short_rows = p->has_cgs2_lds && m <= 256;
    if (p->has_tree) {
        const long long b = std::min<long long>(n, 16);        // the widest tree panel of this operand
        p->tree_in_lds = gs_fused_lds_bytes(esz, std::min<long long>(p->tree_chunk, m), b) <= QR_LDS_BUDGET;
        p->tree_top_in_lds = gs_fused_lds_bytes(esz, p->tree_chunks * b, b) <= QR_LDS_BUDGET;
    }
}

template <class T>
int qr_panel_launch(qil_context* ctx, int kind, long long m, int b, T* P, long long lda, T* R, long long ldr, const double* ref_norm) {
    switch (kind) {
        case QIL_QR_PANEL_TREE: return tsqr_panel<T>(ctx, m, b, P, lda, R, ldr, ref_norm);
        case QIL_QR_PANEL_HH: return hh_panel_launch<T>(ctx, P, lda, m, b, R, ldr, ref_norm);
        default: return gs_fused_launch<T>(ctx, 1u, P, lda, m, b, R, ldr, ref_norm, 0LL);
    }
}

// Thin QR with non-negative diagonal (qr(...; positive=true), rsvd.jl:83,90,94).
//   * small panels: ONE launch (gs_fused);
//   * otherwise blocked CGS2: panels of 16 columns are projected against all previous columns with two
//     MFMA GEMMs per pass (C = Q^H P, then P -= Q C in the second GEMM's epilogue) and orthonormalised internally by gs_fused -- the work is
//     spread over the chip by the GEMMs and the launch count drops from ~5 n to ~7 n / 16.
// Which of these runs, and with which panel kernels, is qr_plan's decision.
template <class T>
int qr_impl(qil_context* ctx, long long m, long long n, T* A, long long lda, T* R, long long ldr, bool* orthonormal, void** rinv) {
    if (orthonormal) *orthonormal = false;
    qil_qr_plan_info p;
    qr_plan(sizeof(T) == 16, m, n, &p);
    qil_qr_report* const rep = ctx->qr_report;               // null outside qil_qr_host
    if (rep) rep->plan = p;
    if (p.cholesky_eligible) {
        if (ctx->cholqr_skip > 0) {
            --ctx->cholqr_skip;
            if (rep) rep->cholesky = 5;
        } else {
            bool done = false;
            QIL_TRY(cholqr2<T>(ctx, m, n, A, lda, R, ldr, &done, orthonormal, rinv));
            if (done) return QIL_OK;
            ctx->cholqr_skip = 8;
        }
    }
    if (p.route == QIL_QR_SINGLE_TREE) {
        void* nb0 = nullptr;
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)n * sizeof(double), &nb0));
        QIL_TRY(col_norms_any<T>(ctx, A, lda, m, n, (double*)nb0));
        QIL_TRY(tsqr_panel<T>(ctx, m, (int)n, A, lda, R, ldr, (const double*)nb0));
        qil_ctx_free(ctx, nb0);
        return QIL_OK;
    }
    if (p.route != QIL_QR_BLOCKED) return qr_panel_launch<T>(ctx, p.panel_kind, m, (int)n, A, lda, R, ldr, (const double*)nullptr);
    const int PB = p.panel_width;
    // (the n x n window only: R may sit inside a wider buffer whose rows beyond n are not this call's)
    if (R) QIL_TRY(qil_dev_zero2d(ctx, R, (size_t)ldr * sizeof(T), (size_t)n * sizeof(T), (size_t)n));
    void *cbuf = nullptr, *nbuf = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)n * sizeof(double), &nbuf));
    // original column norms, measured before any projection (reference for the dependence test)
    QIL_TRY(col_norms_any<T>(ctx, A, lda, m, n, (double*)nbuf));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(n * PB) * sizeof(T), &cbuf));
    T* C = static_cast<T*>(cbuf);
    const int opH = sizeof(T) == 16 ? 2 : 1;
    for (long long j0 = 0; j0 < n; j0 += PB) {
        const int b = (int)std::min<long long>(PB, n - j0);
        T* P = A + lda * j0;
        for (int pass = 0; pass < 2 && j0 > 0; ++pass) {
            QIL_TRY(gemm_dispatch<T>(ctx, opH, 0, j0, b, m, A, lda, P, lda, C, n));      // C = Q^H P
            gemm_batch proj;
            proj.subtract = 1;
            QIL_TRY(gemm_dispatch<T>(ctx, 0, 0, m, b, j0, A, lda, C, n, P, lda, proj));  // P -= Q C
            if (R)
                QIL_TRY((qil_klaunch<add_block_k<T>>(ctx, dim3(8), dim3(256), 0, R + ldr * j0, ldr, (const T*)C, n, (int)j0, b)));
        }
        // intra-panel CGS2 (one launch); its b x b triangular factor goes straight to R[j0:, j0:]
        T* Rjj = R ? R + j0 + ldr * j0 : (T*)nullptr;
        QIL_TRY(qr_panel_launch<T>(ctx, b == PB ? p.panel_kind : p.last_panel_kind, m, b, P, lda, Rjj, ldr, (const double*)nbuf + j0));
    }
    QIL_HIP(hipGetLastError());
    qil_ctx_free(ctx, cbuf);
    qil_ctx_free(ctx, nbuf);
    return QIL_OK;
}

// ------------------------------------------------------------------ device copies / fills as (combinable) kernels
// hipMemcpyAsync / hipMemsetAsync inside a truncation chain are separate commands of the stream: in a lock-step batch they
// would be issued once per chain (3-4 us each, one after another).  As kernels they ride the combined launches.
__device__ __forceinline__ void copy2d_body(const uint3 blockIdx, const uint3 gridDim, double* __restrict__ dst, long long dpitch,
                                            const double* __restrict__ src, long long spitch, long long w, long long h) {
    // pitches and width in 8-byte words
    const long long total = w * h;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t % w, c = t / w;
        dst[r + dpitch * c] = src[r + spitch * c];
    }
}
struct copy2d_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        copy2d_body(b, g, a...);
    }
};
__device__ __forceinline__ void zero2d_body(const uint3 blockIdx, const uint3 gridDim, unsigned* __restrict__ dst, long long pitch,
                                            long long w, long long h) {
    // pitch and width in 4-byte words
    const long long total = w * h;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        dst[(t % w) + pitch * (t / w)] = 0u;
}
struct zero2d_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        zero2d_body(b, g, a...);
    }
};

// A small block of device memory into pinned host memory, then the ticket behind it (system-scope release): the host polls
// the ticket word instead of issuing a copy command and synchronising the stream, and in a lock-step batch the read-backs of
// the chains of a group are ONE launch instead of one copy command + event per chain on the stream they share.
__device__ __forceinline__ void read_back_body(const uint3, const uint3, const unsigned* __restrict__ src, int nwords, unsigned* __restrict__ dst,
                                               unsigned long long* __restrict__ ticket_word, unsigned long long ticket) {
    for (int t = threadIdx.x; t < nwords; t += blockDim.x) dst[t] = src[t];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(ticket_word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
struct read_back_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        read_back_body(b, g, a...);
    }
};

}  // namespace

int qil_read_back_post(qil_context* ctx, const void* dev_src, size_t bytes, uint64_t* ticket) {
    QIL_REQUIRE(bytes > 0 && bytes <= qil_context::kRbSlotBytes && (bytes & 3) == 0 && ((uintptr_t)dev_src & 3) == 0, QIL_EINVAL_ARG,
                "read-back of %zu bytes does not fit a slot", bytes);
    if (!ctx->rb_host) {
        QIL_HIP(hipHostMalloc(&ctx->rb_host, qil_context::kRbSlots * qil_context::kRbSlotBytes + 64, hipHostMallocMapped | hipHostMallocCoherent));
        memset(ctx->rb_host, 0, qil_context::kRbSlots * qil_context::kRbSlotBytes + 64);
    }
    const uint64_t t = ++ctx->rb_ticket;
    char* base = static_cast<char*>(ctx->rb_host);
    unsigned* slot = reinterpret_cast<unsigned*>(base + (t % qil_context::kRbSlots) * qil_context::kRbSlotBytes);
    unsigned long long* word = reinterpret_cast<unsigned long long*>(base + qil_context::kRbSlots * qil_context::kRbSlotBytes);
    *ticket = t;
    return qil_klaunch<read_back_k>(ctx, dim3(1), dim3(256), 0, static_cast<const unsigned*>(dev_src), (int)(bytes / 4), slot, word,
                                    (unsigned long long)t);
}
int qil_read_back_wait(qil_context* ctx, uint64_t ticket, void* host_dst, size_t bytes) {
    char* base = static_cast<char*>(ctx->rb_host);
    const unsigned long long* word = reinterpret_cast<const unsigned long long*>(base + qil_context::kRbSlots * qil_context::kRbSlotBytes);
    const auto t0 = std::chrono::steady_clock::now();
    long long spins = 0;
    if (ctx->lockstep) {                                         // (sleeps; the group's launcher watches the word)
        const int pst = qil_lockstep_park(ctx, word, ticket);
        if (pst != QIL_OK)
            return qil_fail(pst, "read-back %llu of a lock-step chain did not arrive (a combined launch failed, or 60 s passed)", (unsigned long long)ticket);
    }
    while (__atomic_load_n(word, __ATOMIC_ACQUIRE) < ticket) {
        __builtin_ia32_pause();
        if ((++spins & 0xfffff) == 0) {                          // a launch that never ran must not hang the caller
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
                return qil_fail(QIL_EHIP, "read-back %llu did not arrive within 60 s (device error?)", (unsigned long long)ticket);
            if (!ctx->lockstep) {
                const hipError_t e = hipStreamQuery(ctx->stream);
                if (e != hipSuccess && e != hipErrorNotReady) return qil_fail(QIL_EHIP, "stream error while waiting for a read-back: %s", hipGetErrorString(e));
            }
        }
    }
    memcpy(host_dst, base + (ticket % qil_context::kRbSlots) * qil_context::kRbSlotBytes, bytes);
    ctx->rb_done = std::max(ctx->rb_done, (uint64_t)ticket);
    if (ctx->dbg_times) {
        ctx->dbg_rb_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ++ctx->dbg_rb_n;
    }
    return QIL_OK;
}
int qil_read_back(qil_context* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    if (bytes == 0) return QIL_OK;
    if (bytes > qil_context::kRbSlotBytes || (bytes & 3) || ((uintptr_t)dev_src & 3)) {
        QIL_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, qil_stream(ctx)));
        QIL_HIP(qil_stream_sync(ctx));
        if (ctx->rb_done == ctx->rb_ticket) ctx->rb_done = ++ctx->rb_ticket;   // (nothing posted is outstanding: everything launched so far is complete)
        return QIL_OK;
    }
    uint64_t t = 0;
    QIL_TRY(qil_read_back_post(ctx, dev_src, bytes, &t));
    return qil_read_back_wait(ctx, t, host_dst, bytes);
}

int qil_stage_acquire(qil_context* ctx, size_t bytes, void** host, void** dev, int* slot) {
    QIL_REQUIRE(bytes <= qil_context::kStSlotBytes, QIL_EINVAL_ARG, "staged upload of %zu bytes exceeds the slot size", bytes);
    if (!ctx->st_host) {
        const size_t tot = qil_context::kStSlots * qil_context::kStSlotBytes;
        QIL_HIP(hipHostMalloc(&ctx->st_host, tot, hipHostMallocMapped | hipHostMallocCoherent));
        QIL_HIP(hipMalloc(&ctx->st_dev, tot));
    }
    const int k = ctx->st_next;
    ctx->st_next = (k + 1) % qil_context::kStSlots;
    if (ctx->st_used[k] && ctx->rb_done <= ctx->st_born[k]) {    // no read-back posted after its consumers has come back yet
        unsigned word = 0;
        QIL_TRY(qil_read_back(ctx, &word, ctx->st_dev, sizeof(word)));
    }
    ctx->st_used[k] = false;
    *host = static_cast<char*>(ctx->st_host) + (size_t)k * qil_context::kStSlotBytes;
    *dev = static_cast<char*>(ctx->st_dev) + (size_t)k * qil_context::kStSlotBytes;
    *slot = k;
    return QIL_OK;
}
int qil_stage_push(qil_context* ctx, int slot, size_t bytes) {
    const size_t off = (size_t)slot * qil_context::kStSlotBytes;
    return qil_dev_copy(ctx, static_cast<char*>(ctx->st_dev) + off, static_cast<const char*>(ctx->st_host) + off, (bytes + 7) & ~(size_t)7);
}
void qil_stage_commit(qil_context* ctx, int slot) {
    ctx->st_born[slot] = ctx->rb_ticket;
    ctx->st_used[slot] = true;
}

int qil_dev_copy2d(qil_context* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
    if (width == 0 || height == 0) return QIL_OK;
    const bool words = ((dpitch | spitch | width | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src) & 7) == 0;
    if (!words || width * height > ((size_t)64 << 20)) {         // odd shapes / bulk data: the copy engine path
        QIL_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, qil_stream(ctx)));
        return QIL_OK;
    }
    const long long total = (long long)(width / 8) * (long long)height;
    return qil_klaunch<copy2d_k>(ctx, dim3((unsigned)std::min<long long>((total + 255) / 256, 2048)), dim3(256), 0,
                                 static_cast<double*>(dst), (long long)(dpitch / 8), static_cast<const double*>(src),
                                 (long long)(spitch / 8), (long long)(width / 8), (long long)height);
}
int qil_dev_copy(qil_context* ctx, void* dst, const void* src, size_t bytes) {
    return qil_dev_copy2d(ctx, dst, bytes, src, bytes, bytes, 1);
}
int qil_dev_zero2d(qil_context* ctx, void* dst, size_t pitch, size_t width, size_t height) {
    if (width == 0 || height == 0) return QIL_OK;
    const bool words = ((pitch | width | (size_t)(uintptr_t)dst) & 3) == 0;
    if (!words || width * height > ((size_t)64 << 20)) {
        QIL_HIP(hipMemset2DAsync(dst, pitch, 0, width, height, qil_stream(ctx)));
        return QIL_OK;
    }
    const long long total = (long long)(width / 4) * (long long)height;
    return qil_klaunch<zero2d_k>(ctx, dim3((unsigned)std::min<long long>((total + 255) / 256, 2048)), dim3(256), 0,
                                 static_cast<unsigned*>(dst), (long long)(pitch / 4), (long long)(width / 4), (long long)height);
}
int qil_dev_zero(qil_context* ctx, void* dst, size_t bytes) { return qil_dev_zero2d(ctx, dst, bytes, bytes, 1); }

namespace {

// ------------------------------------------------------------------ misc kernels
template <class T>
__device__ __forceinline__ void scale_kernel_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ A, long long lda, long long m, long long n,
                             const double* __restrict__ s, int side) {
    const long long total = m * n;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long i = t % m, j = t / m;
        A[i + lda * j] = scale_t(A[i + lda * j], side ? s[j] : s[i]);
    }
}
template <class T>
struct scale_kernel_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        scale_kernel_body<T>(b, g, a...);
    }
};

// counter-based N(0,1): element i draws from hash(seed, 2i), hash(seed, 2i+1) via Box-Muller
__global__ void fill_normal_kernel(double* __restrict__ p, long long n, uint64_t seed, double scale) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n;
         t += (long long)gridDim.x * blockDim.x) {
        const uint64_t h1 = splitmix64(seed ^ splitmix64(2ull * (uint64_t)t));
        const uint64_t h2 = splitmix64(seed ^ splitmix64(2ull * (uint64_t)t + 1ull));
        const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740993.0);  // (0, 1)
        const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);          // [0, 1)
        p[t] = scale * sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    }
}

}  // namespace

// ------------------------------------------------------------------ exported (internal) entry points
int qil_dev_gemm(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                 const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc) {
    if (dtype == QIL_C64)
        return gemm_dispatch<c64>(ctx, opA, opB, m, n, k, (const c64*)A, lda, (const c64*)B, ldb, (c64*)C, ldc);
    // for real data H == T and conj == N
    static const int real_op[4] = {0, 1, 1, 0};
    return gemm_dispatch<double>(ctx, real_op[opA & 3], real_op[opB & 3], m, n, k, (const double*)A, lda,
                                 (const double*)B, ldb, (double*)C, ldc);
}

int qil_dev_gemm_skinny(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                        const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc) {
    gemm_batch bt;
    bt.skinny_m = 1;
    if (dtype == QIL_C64)
        return gemm_dispatch<c64>(ctx, opA, opB, m, n, k, (const c64*)A, lda, (const c64*)B, ldb, (c64*)C, ldc, bt);
    static const int real_op[4] = {0, 1, 1, 0};
    return gemm_dispatch<double>(ctx, real_op[opA & 3], real_op[opB & 3], m, n, k, (const double*)A, lda,
                                 (const double*)B, ldb, (double*)C, ldc, bt);
}

// sizes, op codes and leading dimensions of a host-facing GEMM call: a leading dimension smaller than the stored rows of its
// operand would make the kernel read (lda, ldb) or write (ldc) outside the allocation
static int gemm_check_args(int opA, int opB, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc) {
    QIL_REQUIRE(m >= 1 && n >= 1 && k >= 1, QIL_EINVAL_ARG, "gemm: empty operand");
    QIL_REQUIRE(opA >= 0 && opA <= 3 && opB >= 0 && opB <= 3, QIL_EINVAL_ARG, "gemm: bad op code");
    const int64_t a_rows = (opA == 0 || opA == 3) ? m : k, b_rows = (opB == 0 || opB == 3) ? k : n;
    QIL_REQUIRE(lda >= a_rows, QIL_EINVAL_ARG, "gemm: lda %lld is smaller than the %lld stored rows of A", (long long)lda, (long long)a_rows);
    QIL_REQUIRE(ldb >= b_rows, QIL_EINVAL_ARG, "gemm: ldb %lld is smaller than the %lld stored rows of B", (long long)ldb, (long long)b_rows);
    QIL_REQUIRE(ldc >= m, QIL_EINVAL_ARG, "gemm: ldc %lld is smaller than the %lld rows of C", (long long)ldc, (long long)m);
    return QIL_OK;
}

// C = opA(A) * opB(B) on host operands (column-major): utility / test hook for the MFMA GEMM
extern "C" int qil_gemm(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                        const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc) {
    QIL_REQUIRE(ctx && A && B && C, QIL_EINVAL_ARG, "gemm: null argument");
    QIL_TRY(gemm_check_args(opA, opB, m, n, k, lda, ldb, ldc));
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const size_t e = qil_elem_size(dtype);
    const int64_t a_cols = (opA == 0 || opA == 3) ? k : m, b_cols = (opB == 0 || opB == 3) ? n : k;
    void *dA = nullptr, *dB = nullptr, *dC = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(lda * a_cols) * e, &dA));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(ldb * b_cols) * e, &dB));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(ldc * n) * e, &dC));
    QIL_HIP(hipMemcpyAsync(dA, A, (size_t)(lda * a_cols) * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(hipMemcpyAsync(dB, B, (size_t)(ldb * b_cols) * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_TRY(qil_dev_zero(ctx, dC, (size_t)(ldc * n) * e));
    QIL_HIP(qil_stream_sync(ctx));
    QIL_TRY(qil_dev_gemm(ctx, dtype, opA, opB, m, n, k, dA, lda, dB, ldb, dC, ldc));
    QIL_TRY(qil_read_back(ctx, C, dC, (size_t)(ldc * n) * e));
    qil_ctx_free(ctx, dA);
    qil_ctx_free(ctx, dB);
    qil_ctx_free(ctx, dC);
    return QIL_OK;
}

// What the dispatch would decide for this product (testing hook; host only)
extern "C" int qil_gemm_plan(int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc,
                             int64_t count, int64_t c_bs, int has_cmap, int skinny_m, qil_gemm_plan_info* plan) {
    QIL_REQUIRE(plan, QIL_EINVAL_ARG, "gemm: null argument");
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "gemm: bad dtype %d", dtype);
    QIL_TRY(gemm_check_args(opA, opB, m, n, k, lda, ldb, ldc));
    QIL_REQUIRE(count >= 1 && count <= 65535, QIL_EINVAL_ARG, "gemm: batch count %lld exceeds the grid limit", (long long)count);
    static const int real_op[4] = {0, 1, 1, 0};   // for real data H == T and conj == N
    if (dtype == QIL_F64) opA = real_op[opA], opB = real_op[opB];
    gemm_plan(dtype == QIL_C64, opA, opB, m, n, k, lda, ldb, ldc, count, c_bs, has_cmap != 0, skinny_m, plan);
    return QIL_OK;
}

// The batched and epilogue forms on host operands (testing hook): whole parent buffers up, gemm_dispatch on base + off, whole C down
extern "C" int qil_gemm_batched_host(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                                     const qil_gemm_host_operand* A, const qil_gemm_host_operand* B, const qil_gemm_host_operand* C,
                                     int64_t count, int subtract, int skinny_m, const uint8_t* b_sel, int64_t b_sel_step,
                                     int64_t b_sel_stride, const int32_t* cmap, int64_t cmap_blk) {
    QIL_REQUIRE(ctx && A && B && C && A->base && B->base && C->base, QIL_EINVAL_ARG, "gemm: null argument");
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "gemm: bad dtype %d", dtype);
    QIL_TRY(gemm_check_args(opA, opB, m, n, k, A->ld, B->ld, C->ld));
    QIL_REQUIRE(count >= 1, QIL_EINVAL_ARG, "gemm: empty batch");
    QIL_REQUIRE(count <= 65535, QIL_EINVAL_ARG, "gemm: batch count %lld exceeds the grid limit", (long long)count);
    // every element the kernels touch lies inside its parent buffer
    QIL_REQUIRE(A->off >= 0 && A->bs >= 0 && B->off >= 0 && B->bs >= 0 && C->off >= 0 && C->bs >= 0 && b_sel_step >= 0 && b_sel_stride >= 0,
                QIL_EINVAL_ARG, "gemm: negative offset or stride");
    const int64_t a_rows = (opA == 0 || opA == 3) ? m : k, a_cols = (opA == 0 || opA == 3) ? k : m;
    const int64_t b_rows = (opB == 0 || opB == 3) ? k : n, b_cols = (opB == 0 || opB == 3) ? n : k;
    int64_t sel_max = 0, c_cols = n;
    if (b_sel)
        for (int64_t b = 0; b < count; ++b) sel_max = std::max<int64_t>(sel_max, b_sel[b * b_sel_step]);
    if (cmap) {
        QIL_REQUIRE(cmap_blk >= 1 && n % cmap_blk == 0, QIL_EINVAL_ARG, "gemm: cmap needs n (%lld) to be a multiple of its block (%lld)",
                    (long long)n, (long long)cmap_blk);
        int64_t blk_max = 0;
        for (int64_t g = 0; g < count * (n / cmap_blk); ++g) {
            QIL_REQUIRE(cmap[g] >= 0, QIL_EINVAL_ARG, "gemm: negative cmap entry");
            blk_max = std::max<int64_t>(blk_max, cmap[g]);
        }
        c_cols = (blk_max + 1) * cmap_blk;
    }
    QIL_REQUIRE(A->off + (count - 1) * A->bs + (a_rows - 1) + A->ld * (a_cols - 1) < A->elems, QIL_EINVAL_ARG, "gemm: A reaches beyond its buffer");
    QIL_REQUIRE(B->off + (count - 1) * B->bs + sel_max * b_sel_stride + (b_rows - 1) + B->ld * (b_cols - 1) < B->elems, QIL_EINVAL_ARG,
                "gemm: B reaches beyond its buffer");
    QIL_REQUIRE(C->off + (count - 1) * C->bs + (m - 1) + C->ld * (c_cols - 1) < C->elems, QIL_EINVAL_ARG, "gemm: C reaches beyond its buffer");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const size_t e = qil_elem_size(dtype);
    void *dA = nullptr, *dB = nullptr, *dC = nullptr, *dsel = nullptr, *dmap = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)A->elems * e, &dA));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)B->elems * e, &dB));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)C->elems * e, &dC));
    QIL_HIP(hipMemcpyAsync(dA, A->base, (size_t)A->elems * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(hipMemcpyAsync(dB, B->base, (size_t)B->elems * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(hipMemcpyAsync(dC, C->base, (size_t)C->elems * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    gemm_batch bt;
    bt.count = (int)count;
    bt.a_bs = A->bs, bt.b_bs = B->bs, bt.c_bs = C->bs;
    bt.subtract = subtract ? 1 : 0;
    bt.skinny_m = skinny_m ? 1 : 0;
    if (b_sel) {
        const size_t nsel = (size_t)((count - 1) * b_sel_step + 1);
        QIL_TRY(qil_ctx_alloc(ctx, nsel, &dsel));
        QIL_HIP(hipMemcpyAsync(dsel, b_sel, nsel, hipMemcpyHostToDevice, qil_stream(ctx)));
        bt.b_sel = static_cast<const uint8_t*>(dsel), bt.b_sel_step = b_sel_step, bt.b_sel_stride = b_sel_stride;
    }
    if (cmap) {
        const size_t nmap = (size_t)(count * (n / cmap_blk)) * sizeof(int);
        QIL_TRY(qil_ctx_alloc(ctx, nmap, &dmap));
        QIL_HIP(hipMemcpyAsync(dmap, cmap, nmap, hipMemcpyHostToDevice, qil_stream(ctx)));
        bt.cmap = static_cast<const int*>(dmap), bt.cmap_blk = (int)cmap_blk;
    }
    QIL_HIP(qil_stream_sync(ctx));
    if (dtype == QIL_C64) {
        QIL_TRY(gemm_dispatch<c64>(ctx, opA, opB, m, n, k, (const c64*)dA + A->off, A->ld, (const c64*)dB + B->off, B->ld,
                                   (c64*)dC + C->off, C->ld, bt));
    } else {
        static const int real_op[4] = {0, 1, 1, 0};
        QIL_TRY(gemm_dispatch<double>(ctx, real_op[opA], real_op[opB], m, n, k, (const double*)dA + A->off, A->ld,
                                      (const double*)dB + B->off, B->ld, (double*)dC + C->off, C->ld, bt));
    }
    QIL_TRY(qil_read_back(ctx, C->base, dC, (size_t)C->elems * e));
    qil_ctx_free(ctx, dA);
    qil_ctx_free(ctx, dB);
    qil_ctx_free(ctx, dC);
    if (dsel) qil_ctx_free(ctx, dsel);
    if (dmap) qil_ctx_free(ctx, dmap);
    return QIL_OK;
}

// Thin QR with non-negative diagonal on a host operand (m >= n): utility / test hook for the Gram-Schmidt QR
extern "C" int qil_qr_positive(qil_context* ctx, int dtype, int64_t m, int64_t n, const void* A, void* Q, void* R) {
    QIL_REQUIRE(ctx && A && Q && R, QIL_EINVAL_ARG, "qr: null argument");
    QIL_REQUIRE(m >= n && n >= 1, QIL_EINVAL_ARG, "qr: needs m >= n >= 1 (got %lld x %lld)", (long long)m, (long long)n);
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const size_t e = qil_elem_size(dtype);
    void *dA = nullptr, *dR = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(m * n) * e, &dA));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(n * n) * e, &dR));
    QIL_HIP(hipMemcpyAsync(dA, A, (size_t)(m * n) * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    QIL_TRY(qil_dev_qr_positive(ctx, dtype, m, n, dA, m, dR, n, true));
    QIL_HIP(hipMemcpyAsync(Q, dA, (size_t)(m * n) * e, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_TRY(qil_read_back(ctx, R, dR, (size_t)(n * n) * e));
    qil_ctx_free(ctx, dA);
    qil_ctx_free(ctx, dR);
    return QIL_OK;
}

// What qr_impl would decide for this operand (testing hook; host only)
extern "C" int qil_qr_plan(int dtype, int64_t m, int64_t n, qil_qr_plan_info* plan) {
    QIL_REQUIRE(plan, QIL_EINVAL_ARG, "qr: null argument");
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "qr: bad dtype %d", dtype);
    QIL_REQUIRE(m >= n && n >= 1, QIL_EINVAL_ARG, "qr: needs m >= n >= 1 (got %lld x %lld)", (long long)m, (long long)n);
    qr_plan(dtype == QIL_C64, m, n, plan);
    return QIL_OK;
}

// The thin QR on host operands (testing hook): whole parent buffers up, qil_dev_qr_positive on base + off, whole parents down
extern "C" int qil_qr_host(qil_context* ctx, int dtype, int64_t m, int64_t n, void* a_base, int64_t a_elems, int64_t a_off, int64_t lda,
                           void* r_base, int64_t r_elems, int64_t r_off, int64_t ldr, int reorth, int cholesky_skip,
                           qil_qr_report* report) {
    QIL_REQUIRE(ctx && a_base && report, QIL_EINVAL_ARG, "qr: null argument");
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "qr: bad dtype %d", dtype);
    QIL_REQUIRE(m >= n && n >= 1, QIL_EINVAL_ARG, "qr: needs m >= n >= 1 (got %lld x %lld)", (long long)m, (long long)n);
    QIL_REQUIRE(m <= INT32_MAX, QIL_EINVAL_ARG, "qr: %lld rows exceed the panel kernels' row index", (long long)m);
    QIL_REQUIRE(lda >= m, QIL_EINVAL_ARG, "qr: lda %lld is smaller than the %lld rows of A", (long long)lda, (long long)m);
    QIL_REQUIRE(a_off >= 0 && a_off + (m - 1) + lda * (n - 1) < a_elems, QIL_EINVAL_ARG, "qr: A reaches beyond its buffer");
    QIL_REQUIRE(cholesky_skip >= 0, QIL_EINVAL_ARG, "qr: negative cholesky_skip");
    if (r_base) {
        QIL_REQUIRE(ldr >= n, QIL_EINVAL_ARG, "qr: ldr %lld is smaller than the %lld rows of R", (long long)ldr, (long long)n);
        QIL_REQUIRE(r_off >= 0 && r_off + (n - 1) + ldr * (n - 1) < r_elems, QIL_EINVAL_ARG, "qr: R reaches beyond its buffer");
    }
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    ctx->cholqr_skip = cholesky_skip;
    *report = qil_qr_report{};
    struct report_guard {                                    // the pointer never outlives the call, however it ends
        qil_context* c;
        ~report_guard() { c->qr_report = nullptr; }
    } guard{ctx};
    ctx->qr_report = report;
    const size_t e = qil_elem_size(dtype);
    void *dA = nullptr, *dR = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)a_elems * e, &dA));
    QIL_HIP(hipMemcpyAsync(dA, a_base, (size_t)a_elems * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    if (r_base) {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)r_elems * e, &dR));
        QIL_HIP(hipMemcpyAsync(dR, r_base, (size_t)r_elems * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    }
    QIL_HIP(qil_stream_sync(ctx));
    QIL_TRY(qil_dev_qr_positive(ctx, dtype, m, n, static_cast<char*>(dA) + (size_t)a_off * e, lda,
                                dR ? static_cast<char*>(dR) + (size_t)r_off * e : nullptr, ldr, reorth != 0));
    if (r_base) QIL_TRY(qil_read_back(ctx, r_base, dR, (size_t)r_elems * e));
    QIL_TRY(qil_read_back(ctx, a_base, dA, (size_t)a_elems * e));
    qil_ctx_free(ctx, dA);
    if (dR) qil_ctx_free(ctx, dR);
    return QIL_OK;
}

// Device-resident timing of the GEMM (operands generated on the device, HIP events): ms per call.
extern "C" int qil_gemm_device_time(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                                    int reps, double* ms_per_call) {
    QIL_REQUIRE(ctx && ms_per_call && reps >= 1, QIL_EINVAL_ARG, "gemm_device_time: bad argument");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const size_t e = qil_elem_size(dtype);
    const int64_t a_rows = (opA == 0 || opA == 3) ? m : k, a_cols = (opA == 0 || opA == 3) ? k : m;
    const int64_t b_rows = (opB == 0 || opB == 3) ? k : n, b_cols = (opB == 0 || opB == 3) ? n : k;
    void *dA = nullptr, *dB = nullptr, *dC = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(a_rows * a_cols) * e, &dA));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(b_rows * b_cols) * e, &dB));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(m * n) * e, &dC));
    QIL_TRY(qil_dev_fill_normal(ctx, dtype, dA, a_rows * a_cols, 11, 1.0));
    QIL_TRY(qil_dev_fill_normal(ctx, dtype, dB, b_rows * b_cols, 12, 1.0));
    QIL_TRY(qil_dev_gemm(ctx, dtype, opA, opB, m, n, k, dA, a_rows, dB, b_rows, dC, m));   // warm-up
    hipEvent_t e0, e1;
    QIL_HIP(hipEventCreate(&e0));
    QIL_HIP(hipEventCreate(&e1));
    QIL_HIP(hipEventRecord(e0, qil_stream(ctx)));
    for (int r = 0; r < reps; ++r) QIL_TRY(qil_dev_gemm(ctx, dtype, opA, opB, m, n, k, dA, a_rows, dB, b_rows, dC, m));
    QIL_HIP(hipEventRecord(e1, qil_stream(ctx)));
    QIL_HIP(hipEventSynchronize(e1));
    float f = 0;
    QIL_HIP(hipEventElapsedTime(&f, e0, e1));
    *ms_per_call = (double)f / reps;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    qil_ctx_free(ctx, dA);
    qil_ctx_free(ctx, dB);
    qil_ctx_free(ctx, dC);
    return QIL_OK;
}

int qil_dev_gemm_batched(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                         const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                         const qil_gemm_batch* b) {
    gemm_batch bt;
    bt.a_bs = b->a_bs;
    bt.b_bs = b->b_bs;
    bt.c_bs = b->c_bs;
    bt.b_sel_step = b->b_sel_step;
    bt.b_sel_stride = b->b_sel_stride;
    static const int real_op[4] = {0, 1, 1, 0};
    // the batch is the grid's y dimension: in pieces of its limit
    for (int64_t b0 = 0; b0 < b->count; b0 += 65535) {
        bt.count = (int)std::min<int64_t>(65535, b->count - b0);
        bt.b_sel = b->b_sel ? b->b_sel + b0 * b->b_sel_step : nullptr;
        if (dtype == QIL_C64)
            QIL_TRY(gemm_dispatch<c64>(ctx, opA, opB, m, n, k, (const c64*)A + b0 * b->a_bs, lda, (const c64*)B + b0 * b->b_bs, ldb,
                                       (c64*)C + b0 * b->c_bs, ldc, bt));
        else
            QIL_TRY(gemm_dispatch<double>(ctx, real_op[opA & 3], real_op[opB & 3], m, n, k, (const double*)A + b0 * b->a_bs, lda,
                                          (const double*)B + b0 * b->b_bs, ldb, (double*)C + b0 * b->c_bs, ldc, bt));
    }
    return QIL_OK;
}

int qil_dev_transpose(qil_context* ctx, int dtype, int conj, int64_t m, int64_t n, const void* A, int64_t lda,
                      void* At, int64_t ldt) {
    if (m == 0 || n == 0) return QIL_OK;
    const unsigned g = (unsigned)std::min<long long>((m * n + 255) / 256, 65536);
    if (dtype == QIL_C64) {
        if (conj)
            QIL_TRY((qil_klaunch<conj_transpose_k<c64, true>>(ctx, dim3(g), dim3(256), 0, (const c64*)A, lda, m, n, (c64*)At, ldt)));
        else
            QIL_TRY((qil_klaunch<conj_transpose_k<c64, false>>(ctx, dim3(g), dim3(256), 0, (const c64*)A, lda, m, n, (c64*)At, ldt)));
    } else {
        QIL_TRY((qil_klaunch<conj_transpose_k<double, false>>(ctx, dim3(g), dim3(256), 0, (const double*)A, lda, m, n, (double*)At, ldt)));
    }
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

int qil_dev_svd(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, void* U,
                int64_t ldu, double* S_host, void* Vh, int64_t ldvh, double negligible_rel) {
    if (dtype == QIL_C64)
        return svd_impl<c64>(ctx, m, n, (c64*)A, lda, (c64*)U, ldu, S_host, (c64*)Vh, ldvh, negligible_rel);
    return svd_impl<double>(ctx, m, n, (double*)A, lda, (double*)U, ldu, S_host, (double*)Vh, ldvh, negligible_rel);
}

int qil_dev_svd_left(qil_context* ctx, int dtype, int64_t p, int64_t q, void* B, int64_t ldb, void* Uiso, int64_t ldu,
                     double* S_host, void* SVh, int64_t ldsvh, double negligible_rel, int* handled, double cert_cutoff,
                     double deflate) {
    if (dtype == QIL_C64)
        return svd_left_mid<c64>(ctx, p, q, static_cast<c64*>(B), ldb, static_cast<c64*>(Uiso), ldu, S_host,
                                 static_cast<c64*>(SVh), ldsvh, negligible_rel, handled, cert_cutoff, deflate);
    return svd_left_mid<double>(ctx, p, q, static_cast<double*>(B), ldb, static_cast<double*>(Uiso), ldu, S_host,
                                static_cast<double*>(SVh), ldsvh, negligible_rel, handled, cert_cutoff, deflate);
}

// thin QR of the tall orientation + the certificate, for operands outside the one-factor SVD's range (>= 640 columns):
// A (m x n, lda) is left intact; on success (*certified) Qout (rows x k, ld rows) / Rout (k x k, ld k) hold the factors of A
// (m >= n) or of A^H (m < n), rows = max(m, n), k = min(m, n)
template <class T>
static int qr_certified_t(qil_context* ctx, long long m, long long n, const T* A, long long lda, double cutoff, T* Qout, T* Rout,
                          bool* certified) {
    const long long rows = std::max(m, n), k = std::min(m, n);
    if (m >= n)
        QIL_TRY(qil_dev_copy2d(ctx, Qout, (size_t)rows * sizeof(T), A, (size_t)lda * sizeof(T), (size_t)m * sizeof(T), (size_t)n));
    else
        QIL_TRY((qil_klaunch<conj_transpose_k<T>>(ctx, dim3((unsigned)std::min<long long>((m * n + 255) / 256, 65536)), dim3(256), 0, A, lda, m, n, Qout, rows)));
    bool known = false;
    void* rinv = nullptr;                                        // R^-1 from CholeskyQR2 for the certificate
    QIL_TRY(qr_impl<T>(ctx, rows, k, Qout, rows, Rout, k, &known, cutoff > 0.0 ? &rinv : nullptr));
    bool ok = true;
    QIL_TRY(qr_reorthogonalise<T>(ctx, rows, k, Qout, rows, Rout, k, known, &rinv, false, &ok));
    *certified = false;
    if (!ok) {
        if (rinv) qil_ctx_free(ctx, rinv);
        return QIL_OK;
    }
    return certify_no_truncation<T>(ctx, Rout, k, (int)k, cutoff, rinv, certified);
}
int qil_dev_set_identity(qil_context* ctx, int dtype, void* V, int64_t ldv, int64_t n) {
    const unsigned g = (unsigned)std::min<long long>((n * n + 255) / 256, 65536);
    if (dtype == QIL_C64) QIL_TRY((qil_klaunch<set_identity_k<c64>>(ctx, dim3(g), dim3(256), 0, static_cast<c64*>(V), ldv, (int)n)));
    else QIL_TRY((qil_klaunch<set_identity_k<double>>(ctx, dim3(g), dim3(256), 0, static_cast<double*>(V), ldv, (int)n)));
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}
int qil_dev_qr_certified(qil_context* ctx, int dtype, int64_t m, int64_t n, const void* A, int64_t lda, double cutoff, void* Qout,
                         void* Rout, bool* certified) {
    if (dtype == QIL_C64)
        return qr_certified_t<c64>(ctx, m, n, static_cast<const c64*>(A), lda, cutoff, static_cast<c64*>(Qout),
                                   static_cast<c64*>(Rout), certified);
    return qr_certified_t<double>(ctx, m, n, static_cast<const double*>(A), lda, cutoff, static_cast<double*>(Qout),
                                  static_cast<double*>(Rout), certified);
}

// |r_jj|^2 of an n x n triangular factor on the device -> host (n <= 1024): what tells a deficient sketch's noise columns apart
template <class T>
__device__ __forceinline__ void diag_abs2_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ R, long long ldr, int n, double* __restrict__ out) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) out[j] = abs2_t(R[j + ldr * j]);
}
template <class T>
struct diag_abs2_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        diag_abs2_body<T>(b, g, a...);
    }
};
int qil_dev_diag_abs2(qil_context* ctx, int dtype, const void* R, int64_t ldr, int64_t n, double* host_out) {
    QIL_REQUIRE(n >= 1 && n <= 1024, QIL_EINVAL_ARG, "diag: n = %lld", (long long)n);
    void* d = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)n * sizeof(double), &d));
    if (dtype == QIL_C64) QIL_TRY((qil_klaunch<diag_abs2_k<c64>>(ctx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const c64*)R, (long long)ldr, (int)n, (double*)d)));
    else QIL_TRY((qil_klaunch<diag_abs2_k<double>>(ctx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const double*)R, (long long)ldr, (int)n, (double*)d)));
    QIL_TRY(qil_read_back(ctx, host_out, d, (size_t)n * sizeof(double)));
    qil_ctx_free(ctx, d);
    return QIL_OK;
}

int qil_dev_qr_positive(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, void* R,
                        int64_t ldr, bool orthonormal) {
    QIL_REQUIRE(m >= n, QIL_EINVAL_ARG, "qr: needs m >= n (got %lld x %lld)", (long long)m, (long long)n);
    bool known = false;
    if (dtype == QIL_C64) {
        QIL_TRY(qr_impl<c64>(ctx, m, n, (c64*)A, lda, (c64*)R, ldr, &known));
        return orthonormal ? qr_reorthogonalise<c64>(ctx, m, n, (c64*)A, lda, (c64*)R, ldr, known, nullptr, false) : QIL_OK;
    }
    QIL_TRY(qr_impl<double>(ctx, m, n, (double*)A, lda, (double*)R, ldr, &known));
    return orthonormal ? qr_reorthogonalise<double>(ctx, m, n, (double*)A, lda, (double*)R, ldr, known, nullptr, false) : QIL_OK;
}

int64_t qil_truncation_rank(const double* S, int64_t n, double cutoff, bool use_cutoff, int64_t maxdim,
                            int64_t mindim) {
    // ITensors / NDTensors truncate! on P = S^2 (descending) [upstream-recall; pinned by the bond
    // dimensions printed in the reference's tutorials, see oracle/linalg.py]
    if (n <= 0) return 0;
    if (!(S[0] > 0.0)) return 1;
    if (n == 1) return 1;
    if (mindim < 1) mindim = 1;
    int64_t k = n;
    double truncerr = 0.0;
    while (k > maxdim) {
        truncerr += S[k - 1] * S[k - 1];
        --k;
    }
    if (use_cutoff) {
        double scale = 0.0;
        for (int64_t i = 0; i < n; ++i) scale += S[i] * S[i];
        if (scale == 0.0) scale = 1.0;
        while (k > mindim && truncerr + S[k - 1] * S[k - 1] <= cutoff * scale) {
            truncerr += S[k - 1] * S[k - 1];
            --k;
        }
    }
    return k < 1 ? 1 : k;
}

int qil_dev_scale(qil_context* ctx, int dtype, int side, int64_t m, int64_t n, void* A, int64_t lda,
                  const double* s_host) {
    if (m == 0 || n == 0) return QIL_OK;
    const int64_t len = side ? n : m;
    void* sd = nullptr;
    int ring_slot = -1;
    if ((size_t)len * sizeof(double) <= qil_context::kStSlotBytes) {   // pinned ring: no synchronisation
        void* hp = nullptr;
        QIL_TRY(qil_stage_acquire(ctx, (size_t)len * sizeof(double), &hp, &sd, &ring_slot));
        memcpy(hp, s_host, (size_t)len * sizeof(double));
        QIL_TRY(qil_stage_push(ctx, ring_slot, (size_t)len * sizeof(double)));
    } else {
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)len * sizeof(double), &sd));
        QIL_HIP(hipMemcpyAsync(sd, s_host, (size_t)len * sizeof(double), hipMemcpyHostToDevice, qil_stream(ctx)));
        QIL_HIP(qil_stream_sync(ctx));  // s_host is caller memory
    }
    const unsigned g = (unsigned)std::min<long long>((m * n + 255) / 256, 65536);
    if (dtype == QIL_C64)
        QIL_TRY((qil_klaunch<scale_kernel_k<c64>>(ctx, dim3(g), dim3(256), 0, (c64*)A, lda, m, n, (const double*)sd, side)));
    else
        QIL_TRY((qil_klaunch<scale_kernel_k<double>>(ctx, dim3(g), dim3(256), 0, (double*)A, lda, m, n, (const double*)sd, side)));
    QIL_HIP(hipGetLastError());
    if (ring_slot >= 0) {
        qil_stage_commit(ctx, ring_slot);
        return QIL_OK;
    }
    qil_ctx_free(ctx, sd);
    return QIL_OK;
}

int qil_dev_fill_normal(qil_context* ctx, int dtype, void* p, int64_t n_elems, uint64_t seed, double scale) {
    const long long nd = n_elems * (dtype == QIL_C64 ? 2 : 1);
    if (nd == 0) return QIL_OK;
    // complex entries: re, im i.i.d. N(0, 1/2) * scale so that E|z|^2 = scale^2
    const double sc = dtype == QIL_C64 ? scale * M_SQRT1_2 : scale;
    hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)std::min<long long>((nd + 255) / 256, 65536)), dim3(256),
                       0, qil_stream(ctx), (double*)p, nd, seed, sc);
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}
