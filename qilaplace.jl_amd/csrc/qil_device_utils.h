// Device-side helpers shared by the dense linear algebra (qil_linalg.hip), the MPO builders (qil_build*.hip), the
// apply (qil_apply.hip), the read-outs (qil_readout.hip), the overlaps (qil_inner.hip), the sampler (qil_sample.hip), the
// Born weights (qil_weight.hip, qil_apply_weight.hip), the restriction (qil_restrict.hip), the sums (qil_sum.hip), the shared
// contraction steps (qil_contract.hip) and the truncation (qil_truncate.hip): the complex scalar type, its arithmetic and its
// parts (re_of / im_of / make_elem / shfl_xor_t), the one K step of a 16 x 16 tile on the f64 MFMA (mfma_step), the splitmix64
// hash, the sampling rule (seeded_uniform, choose), the row sums of both children (children_row_sums), the per-row steps of
// the beam search (beam_keys, beam_child_scale, beam_gather_row, beam_finish_row), DPP cross-lane sums, Jacobi rotations, the in-workgroup one-sided Jacobi sweep loop, and the site table, site lookup
// and stores of the grouped launches; on the host, the dtype switch of a launch (for_elem_type, for_elem_types).  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

namespace qil_dev {

struct c64 {
    double re, im;
};

// The dtype switch of a launch (host): go(element) with a value of the element type, c64 where `complex`; for_elem_types is
// the two-operand form, go(first element, second element).  Returns what go returns.
template <class F>
auto for_elem_type(bool complex, F go) {
    if (complex) return go(c64{});
    return go(double{});
}
template <class F>
auto for_elem_types(bool complex_a, bool complex_b, F go) {
    return for_elem_type(complex_a, [&](auto a) { return for_elem_type(complex_b, [&](auto b) { return go(a, b); }); });
}

__device__ __forceinline__ double conj_t(double v) { return v; }
__device__ __forceinline__ c64 conj_t(c64 v) { return c64{v.re, -v.im}; }
__device__ __forceinline__ double fma_t(double a, double b, double acc) { return fma(a, b, acc); }
__device__ __forceinline__ c64 fma_t(c64 a, c64 b, c64 acc) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
    return acc;
}
__device__ __forceinline__ double abs2_t(double v) { return v * v; }
__device__ __forceinline__ double abs2_t(c64 v) { return v.re * v.re + v.im * v.im; }
__device__ __forceinline__ double scale_t(double v, double s) { return v * s; }
__device__ __forceinline__ c64 scale_t(c64 v, double s) { return c64{v.re * s, v.im * s}; }
__device__ __forceinline__ double sub_t(double a, double b) { return a - b; }
__device__ __forceinline__ c64 sub_t(c64 a, c64 b) { return c64{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ double add_t(double a, double b) { return a + b; }
__device__ __forceinline__ c64 add_t(c64 a, c64 b) { return c64{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ double cmul_add(double acc, double a, double b) { return fma(a, b, acc); }
__device__ __forceinline__ c64 cmul_add(c64 acc, c64 a, c64 b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
    return acc;
}
__device__ __forceinline__ c64 cmul_add(c64 acc, c64 a, double b) {
    acc.re = fma(a.re, b, acc.re);
    acc.im = fma(a.im, b, acc.im);
    return acc;
}
__device__ __forceinline__ c64 cmul_add(c64 acc, double a, c64 b) {
    acc.re = fma(a, b.re, acc.re);
    acc.im = fma(a, b.im, acc.im);
    return acc;
}
__device__ __forceinline__ c64 to_c64(double v) { return c64{v, 0.0}; }
__device__ __forceinline__ c64 to_c64(c64 v) { return v; }
template <class TD>
__device__ __forceinline__ TD cast_elem(double v);
template <>
__device__ __forceinline__ double cast_elem<double>(double v) { return v; }
template <>
__device__ __forceinline__ c64 cast_elem<c64>(double v) { return c64{v, 0.0}; }
template <class TD>
__device__ __forceinline__ TD cast_elem(c64 v) { return v; }
__device__ __forceinline__ double re_of(double v) { return v; }
__device__ __forceinline__ double re_of(c64 v) { return v.re; }
__device__ __forceinline__ double im_of(double) { return 0.0; }
__device__ __forceinline__ double im_of(c64 v) { return v.im; }
// (re, im) as an element of the type the null pointer names; the imaginary part of a real element is dropped
__device__ __forceinline__ double make_elem(double re, double, double*) { return re; }
__device__ __forceinline__ c64 make_elem(double re, double im, c64*) { return c64{re, im}; }
__device__ __forceinline__ double shfl_xor_t(double v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ c64 shfl_xor_t(c64 v, int m) { return c64{__shfl_xor(v.re, m, 64), __shfl_xor(v.im, m, 64)}; }

// ------------------------------------------------------------------ the f64 MFMA tile step
typedef double d4 __attribute__((ext_vector_type(4)));
// one K step of a 16 x 16 tile on v_mfma_f64_16x16x4_f64: D[i][j] += sum_k X[i][k] Y[k][j], lane l supplies x = X[l & 15][l >> 4]
// and y = Y[l >> 4][l & 15] and holds D[(l >> 4) + 4 reg][l & 15]; c64 through the real / imaginary split
template <class T>
__device__ __forceinline__ void mfma_step(T x, T y, d4& rr, d4& ii) {
    rr = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(x), re_of(y), rr, 0, 0, 0);
    if constexpr (sizeof(T) == 16) {
        rr = __builtin_amdgcn_mfma_f64_16x16x4f64(-im_of(x), im_of(y), rr, 0, 0, 0);
        ii = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(x), im_of(y), ii, 0, 0, 0);
        ii = __builtin_amdgcn_mfma_f64_16x16x4f64(im_of(x), re_of(y), ii, 0, 0, 0);
    }
}

// ------------------------------------------------------------------ counter-based random numbers
// splitmix64 finaliser: the hash behind qil_dev_fill_normal's normals and qil_sample's uniforms
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------ the sampling rule of qil_sample and qil_apply_sample
// u_{r,i} = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53, in [0, 1)
__device__ __forceinline__ double seeded_uniform(uint64_t seed, long long r, int n, int i) {
    const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)r * (uint64_t)n + (uint64_t)i));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// The choice of one sample at one site.  q_0 + q_1 <= 0 (a prefix of weight zero reached through rounding): the larger q,
// s = 0 when both are 0, and the probability factor is 0.  The row is rescaled by 1 / sqrt(q_s), or zeroed when q_s <= 0.
__device__ __forceinline__ int choose(double q0, double q1, double u, double& factor, double& scl) {
    const double sum = q0 + q1;
    int s;
    if (sum > 0.0) {
        s = u * sum < q0 ? 0 : 1;
        factor = (s ? q1 : q0) / sum;
    } else {
        s = q1 > q0 ? 1 : 0;
        factor = 0.0;
    }
    const double qs = s ? q1 : q0;
    scl = qs > 0.0 ? 1.0 / sqrt(qs) : 0.0;
    return s;
}

// q_s = Re sum_beta U_s[row, beta] conj(T_s[row, beta]) for both children of a workgroup's Rows rows (qil_sample's GEMM route,
// qil_top_k).  T (rows x 2 chi_r, column s + 2 beta) and U_s = T_s R (rows x chi_r at Us + s rows chi_r), both ld = rows.  Thread
// (r, g) = (threadIdx.x % Rows, threadIdx.x / Rows) sums the columns g, g + Groups, .. of its row; LDS sums the groups in a fixed
// order.  The whole workgroup calls it (one barrier); true with (a, b) = (q_0, q_1) for the group-0 thread of a row below `rows`.
template <int Rows, int Groups, class T>
__device__ __forceinline__ bool children_row_sums(const T* __restrict__ Tm, const T* __restrict__ Us, long long rows, int cr,
                                                  double (&qs)[2][Groups][Rows], double& a, double& b) {
    const int r = threadIdx.x % Rows, g = threadIdx.x / Rows;
    const long long row = (long long)blockIdx.x * Rows + r;
    double q0 = 0.0, q1 = 0.0;
    if (row < rows)
        for (int beta = g; beta < cr; beta += Groups) {
            const T t0 = Tm[row + rows * (2LL * beta)], t1 = Tm[row + rows * (1 + 2LL * beta)];
            const T u0 = Us[row + rows * (long long)beta], u1 = Us[row + rows * ((long long)cr + beta)];
            q0 += re_of(u0) * re_of(t0) + im_of(u0) * im_of(t0);
            q1 += re_of(u1) * re_of(t1) + im_of(u1) * im_of(t1);
        }
    qs[0][g][r] = q0;
    qs[1][g][r] = q1;
    __syncthreads();
    if (g != 0 || row >= rows) return false;
    a = 0.0, b = 0.0;
    for (int j = 0; j < Groups; ++j) a += qs[0][j][r], b += qs[1][j][r];
    return true;
}

// ------------------------------------------------------------------ the per-row steps of the beam search (qil_top_k, qil_apply_top_k)
// Both children of frontier row `row`: q_s < 0 (rounding of a PSD form) or NaN counts as 0; key(2 row + s) = p q_s / (q_0 + q_1),
// the child's weight / the norm, 0 when the sum is not positive.
__device__ __forceinline__ void beam_keys(double q0, double q1, long long row, const double* __restrict__ p,
                                          double* __restrict__ keys, double* __restrict__ q) {
    q0 = fmax(q0, 0.0);
    q1 = fmax(q1, 0.0);
    const double sum = q0 + q1, pr = p[row];
    keys[2 * row] = sum > 0.0 ? pr * (q0 / sum) : 0.0;
    keys[2 * row + 1] = sum > 0.0 ? pr * (q1 / sum) : 0.0;
    q[2 * row] = q0;
    q[2 * row + 1] = q1;
}
// a kept child is scaled by 1 / sqrt(q), zeroed when q <= 0
__device__ __forceinline__ double beam_child_scale(double qq) { return qq > 0.0 ? 1.0 / sqrt(qq) : 0.0; }
// next frontier row j = candidate c (child c & 1 of row c >> 1): g' = g + log(q) / 2, p' = key, the index for the back-walk
__device__ __forceinline__ void beam_gather_row(long long j, int c, double qq, const double* __restrict__ keys,
                                                const double* __restrict__ g, double* __restrict__ gn, double* __restrict__ pn,
                                                int* __restrict__ anc) {
    gn[j] = g[c >> 1] + (qq > 0.0 ? 0.5 * log(qq) : 0.0);
    pn[j] = keys[c];
    anc[j] = c;
}
// Result row j = candidate c at the last site, where a child is one number, the complete product up to e^g: value =
// sgn e^{g + lamp} child (lamp = log |amp|); the bits are the candidate indices walked back (anc: level lvl at lvl * stride).
template <class T>
__device__ __forceinline__ void beam_finish_row(long long j, int c, T child, const double* __restrict__ g,
                                                const int* __restrict__ anc, long long stride, int n, double lamp, double sgn,
                                                double* __restrict__ val, uint8_t* __restrict__ bits) {
    long long row = c >> 1;
    const c64 v = to_c64(scale_t(child, sgn * exp(g[row] + lamp)));
    val[2 * j] = v.re;
    val[2 * j + 1] = v.im;
    bits[j * n + n - 1] = (uint8_t)(c & 1);
    for (int lvl = n - 2; lvl >= 0; --lvl) {
        const int a = anc[lvl * stride + row];
        bits[j * n + lvl] = (uint8_t)(a & 1);
        row = a >> 1;
    }
}

// ------------------------------------------------------------------ block reductions
// Cross-lane sums on the DPP path (no LDS crossbar): quad_perm butterflies inside each quad, then
// row_half_mirror / row_mirror fold the 8- and 16-lane halves; every lane of a 16-lane row ends with the
// row total.  A ds_bpermute-based __shfl_xor costs ~50+ cycles per step; a DPP move costs a VALU slot.
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ double read_lane_d(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
    v = row16_sum(v);
    return (read_lane_d(v, 0) + read_lane_d(v, 16)) + (read_lane_d(v, 32) + read_lane_d(v, 48));
}
// Totals of TWO values over the 64 lanes, both delivered to every lane, for the price of little more than one: a
// v_permlane32_swap folds the halves so that lanes 0-31 carry a and lanes 32-63 carry b, the four DPP steps and one
// v_permlane16_swap reduce each half, a last v_permlane32_swap broadcasts both totals (22 instructions against 2 x 25).
// The whole wave must be active.
__device__ __forceinline__ double swap_fold32(double x, double y) {   // lanes l < 32: x[l] + x[l + 32]; l >= 32: y[l - 32] + y[l]
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void wave_sum2(double& a, double& b) {
    double t = row16_sum(swap_fold32(a, b));
    {   // rows 0 + 1 and 2 + 3
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(t), (unsigned)__double2loint(t), false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(t), (unsigned)__double2hiint(t), false, false);
        t = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
    }
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(t), (unsigned)__double2loint(t), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(t), (unsigned)__double2hiint(t), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
// every lane of a 32-lane half ends with that half's total
__device__ __forceinline__ double half32_sum(double v) {
    v = row16_sum(v);
    const double lo = read_lane_d(v, 0) + read_lane_d(v, 16), hi = read_lane_d(v, 32) + read_lane_d(v, 48);
    return (threadIdx.x & 32) ? hi : lo;
}
template <int G>
__device__ __forceinline__ double group_sum(double v) {
    return G == 16 ? row16_sum(v) : G == 32 ? half32_sum(v) : wave_sum(v);
}

// sums `NV` doubles per thread across a 256-thread workgroup; result valid in all threads
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* lds /* NV * 4 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[i * 4 + wave] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = lds[i * 4 + 0] + lds[i * 4 + 1] + lds[i * 4 + 2] + lds[i * 4 + 3];
}

// ------------------------------------------------------------------ one-sided Jacobi SVD
// One round of the round-robin tournament: workgroup i orthogonalises columns (p, q) of A
// (m x n) and applies the same rotation to V (n x n).
__device__ __forceinline__ void rotate_pair(double& x, double& y, double c, double s, double pr, double) {
    // pr = sign(x.y): the rotation angle is computed for |gamma|
    const double xn = c * x - s * pr * y, yn = s * pr * x + c * y;
    x = xn;
    y = yn;
}
__device__ __forceinline__ void rotate_pair(c64& x, c64& y, double c, double s, double pr, double pi) {
    // x' = c x - s e^{-i phi} y ;  y' = s e^{i phi} x + c y,  e^{i phi} = pr + i pi
    const c64 ey{pr * y.re + pi * y.im, pr * y.im - pi * y.re};  // e^{-i phi} y
    const c64 ex{pr * x.re - pi * x.im, pr * x.im + pi * x.re};  // e^{ i phi} x
    const c64 xn{c * x.re - s * ey.re, c * x.im - s * ey.im};
    const c64 yn{s * ex.re + c * y.re, s * ex.im + c * y.im};
    x = xn;
    y = yn;
}
__device__ __forceinline__ void dot_parts(double x, double y, double& gr, double& gi) {
    gr += x * y;
    (void)gi;
}
__device__ __forceinline__ void dot_parts(c64 x, c64 y, double& gr, double& gi) {
    // conj(x) * y
    gr += x.re * y.re + x.im * y.im;
    gi += x.re * y.im - x.im * y.re;
}

// Rotation that orthogonalises a column pair with alpha = |x|^2, beta = |y|^2, gamma = x^H y = gr + i gi.
// Returns false when the pair already passes |gamma| <= tol |x| |y|.  The rotation is a dependent chain of
// double-precision sqrt / divide sequences executed once per pair per round -- on the latency-bound
// in-LDS paths it IS the round time, so it is kept to one divide, one sqrt + divide and one rsqrt
// (real: |gamma| and its sign need neither a sqrt nor a divide).
// 1 / sqrt(x) to within an ulp: the library rsqrt plus one Newton step (3 FMAs).  The rotations must be
// unitary to rounding level -- a 2-3 ulp bias in c accumulates over the thousands of rotations V receives.
__device__ __forceinline__ double rsqrt_refined(double x) {
    const double y = rsqrt(x);
    return y * fma(-0.5 * x * y, y, 1.5);
}

// 1 / x from the hardware reciprocal plus one Newton step (2 FMAs): the IEEE divide sequence is ~4x longer
// and sits on the critical path of every rotation.
__device__ __forceinline__ double rcp_refined(double x) {
    const double y = __builtin_amdgcn_rcp(x);
    return y * fma(-x, y, 2.0);
}

// kQuadraticOff: once every pair a sweep meets is already orthogonal to this relative level BEFORE its rotation, that sweep
// (quadratic convergence) leaves all of them at rounding level: the iteration stops there instead of spending one more
// sweep on a handful of 1e-15-level rotations and another one on finding nothing to do.  `big` reports whether this
// pair was above that level.
constexpr double kQuadraticOff = 1e-9;
// ... but the argument needs SMALL angles.  A pair of (nearly) equal norms turns by up to 45 degrees however small its overlap
// is, and such a turn hands the overlaps that its two columns still have with every other column on to pairs the sweep has
// already visited -- at first order.  A sweep that meets only overlaps below kQuadraticOff can then leave 1e-11 behind: an operand
// with a KEPT cluster of equal singular values (75 values at 1e-3 below a flat spectrum, 300 columns) came out with
// max |Q^H Q - 1| = 2.5e-11 between cluster columns and the others.  So a pair that is ROTATED by more than kSmallAngle keeps
// the iteration going like one above kQuadraticOff; the last sweep then turns by less than that, and what it leaves is below
// kSmallAngle * kQuadraticOff.  (A cluster stops turning once its pairs are below tol, which they reach like any other pair.)
// ONLY the rounds of the one-factor SVD of the gauge sweeps honour kSmallAngle so far (svd_left_mid of qil_linalg.hip: the
// vector rounds jacobi_block_round_nov and the Gram rounds gram_block_round, where the defect was measured).  The general SVD
// (jacobi_pair, jacobi_fused, the block Jacobi), jacobi_sweeps below, the spectra and the builders still stop on kQuadraticOff
// alone: `big` of jacobi_rotation / rotation_fast does not know the angle.
constexpr double kSmallAngle = 1e-4;
__device__ __forceinline__ bool turns_far(double al, double be, double g2) {
    const double d = be - al;
    return 4.0 * g2 > (kSmallAngle * kSmallAngle) * (d * d);             // |tan 2 theta| = 2 |g| / |be - al|
}
// Rank-deficient operands (every product bond before its truncation) leave columns that are pure rounding residue:
// |a|^2 below 1e-30 |A|_F^2.  Such a column has no direction to converge to -- each rotation of the genuine columns
// re-randomises it -- and keeps full sweeps going (builder slices: 14.7 -> 4.5 sweeps when it is left alone).  When the
// caller truncates with a cutoff these columns are far below it (the threshold also stays 100x under the cutoff), so
// pairs involving one are skipped; without a cutoff the threshold is 0 and nothing is skipped.
constexpr double kNegligibleColumn = 1e-30;

template <bool CX>
__device__ __forceinline__ bool jacobi_rotation(double al, double be, double gr, double gi, double tol,
                                                double& c, double& s, double& pr, double& pi, bool& big) {
    double half_inv_g;
    big = (gr * gr + gi * gi) > kQuadraticOff * kQuadraticOff * al * be;
    if (CX) {
        const double g2 = gr * gr + gi * gi;
        if (!(g2 > tol * tol * al * be) || g2 == 0.0) return false;
        const double inv_g = rsqrt_refined(g2);
        pr = gr * inv_g;
        pi = gi * inv_g;
        half_inv_g = 0.5 * inv_g;
    } else {
        const double g = fabs(gr);
        if (!(g * g > tol * tol * al * be) || g == 0.0) return false;
        pr = gr >= 0 ? 1.0 : -1.0;
        pi = 0.0;
        half_inv_g = 0.5 * rcp_refined(g);
    }
    // t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)); its accuracy only decides how well THIS pair is annihilated,
    // unitarity rests on c alone (s = c t, c = 1 / sqrt(1 + t^2) to an ulp)
    const double zeta = (be - al) * half_inv_g;
    const double az = fmin(fabs(zeta), 1e150);
    const double u = fma(az, az, 1.0);
    const double t = (zeta >= 0 ? 1.0 : -1.0) * rcp_refined(az + u * rsqrt_refined(u));
    c = rsqrt_refined(fma(t, t, 1.0));
    s = c * t;
    return true;
}

// Rotation of a column pair from |x|^2 = al, |y|^2 = be, x^H y = gr + i gi:  x' = c x - conj(sg) y,  y' = sg x + c y with
// sg = s e^{i phi} = (sr, si), e^{i phi} = g / |g|, s signed by be - al; sabs = |sg|, gabs ~ |g|.
// The dependent chain of this computation sits on the critical path of every inner round, so it is kept short: the angle comes
// from the raw hardware reciprocal square roots (relative error ~1e-8, which only decides how completely THIS pair is
// annihilated -- quadratic convergence absorbs it), and unitarity, which must hold to rounding because the errors of
// thousands of rotations add up in the singular values, is restored exactly afterwards: with eps = c0^2 + |sg0|^2 - 1
// (|eps| < 1e-6) both are scaled by 1 / sqrt(1 + eps) = 1 - eps / 2 + 3 eps^2 / 8 + O(eps^3 < 1e-18).
template <bool CX>
__device__ __forceinline__ bool rotation_fast(double al, double be, double gr, double gi, double tol, double& c, double& sr,
                                              double& si, double& sabs, double& gabs, bool& big) {
    const double g2 = CX ? fma(gr, gr, gi * gi) : gr * gr;
    const double ab = al * be;
    big = g2 > kQuadraticOff * kQuadraticOff * ab;
    if (!(g2 > tol * tol * ab) || g2 == 0.0) return false;
    const double d = be - al;
    const double rh = __builtin_amdgcn_rsq(fma(d, d, 4.0 * g2));
    const double c2 = fma(0.5 * fabs(d), rh, 0.5);
    const double rc = __builtin_amdgcn_rsq(c2);
    const double c0 = c2 * rc;
    const double q = copysign(rh * rc, d);            // sg0 = q g
    const double sr0 = q * gr, si0 = CX ? q * gi : 0.0;
    const double s02 = CX ? fma(sr0, sr0, si0 * si0) : sr0 * sr0;
    const double eps = fma(c0, c0, s02 - 1.0);
    const double f = fma(eps, fma(eps, 0.375, -0.5), 1.0);
    c = c0 * f;
    sr = sr0 * f;
    si = si0 * f;
    // |sg| and |g| only feed the carried norms (re-taken from the data at every staging): raw accuracy is enough
    gabs = CX ? g2 * __builtin_amdgcn_rsq(g2) : fabs(gr);
    sabs = fabs(q) * gabs * f;
    return true;
}
__device__ __forceinline__ void rotate_pair_sg(double& x, double& y, double c, double sr, double) {
    const double xn = fma(c, x, -sr * y), yn = fma(sr, x, c * y);
    x = xn;
    y = yn;
}
__device__ __forceinline__ void rotate_pair_sg(c64& x, c64& y, double c, double sr, double si) {
    // x' = c x - conj(sg) y ;  y' = sg x + c y
    const c64 xn{fma(c, x.re, -fma(sr, y.re, si * y.im)), fma(c, x.im, -fma(sr, y.im, -si * y.re))};
    const c64 yn{fma(c, y.re, fma(sr, x.re, -si * x.im)), fma(c, y.im, fma(sr, x.im, si * x.re))};
    x = xn;
    y = yn;
}

// Whole one-sided Jacobi SVD iteration in ONE launch of ONE 1024-thread workgroup: V = I, sweeps of the
// round-robin tournament until no pair rotates, then the column norms.  Each wave owns whole column
// pairs (lanes stride over rows, shuffle reductions), pairs of a round are disjoint, rounds are
// separated by a workgroup barrier.  Used when the rotated side is small (<= 128 columns): there the
// multi-launch form is bounded by ~(n-1) x sweeps kernel boundaries, not by work.  When A and V fit
// the CU's 160 KiB LDS (LDS = true) they are staged there for the whole iteration, so every round
// trip of the rotation is an LDS access instead of an L2 one.
template <class T, int G, int NT = 1024>
__device__ __forceinline__ void jacobi_sweeps(T* A, int lda, int m, T* V, int ldv, int n, double tol,
                                              int max_sweeps, int* s_rot, double negligible = 0.0) {
    // a column pair is owned by a group of G lanes (16 = one DPP row, or the whole wave); NT = workgroup size
    const int tid = threadIdx.x, lane = tid & (G - 1), wave = tid / G;
    constexpr int NW = NT / G;
    const int npad = n + (n & 1);
    for (int sweep = 0; sweep < max_sweeps && n > 1; ++sweep) {
        if (tid == 0) *s_rot = 0;
        __syncthreads();
        for (int round = 0; round < npad - 1; ++round) {
            for (int i = wave; i < npad / 2; i += NW) {
                int p, q;
                if (i == 0) {
                    p = npad - 1;
                    q = round;
                } else {
                    // both sums lie in [0, 2 (npad - 1)): one conditional subtraction, not a runtime modulo
                    p = round + i;
                    q = round + npad - 1 - i;
                    if (p >= npad - 1) p -= npad - 1;
                    if (q >= npad - 1) q -= npad - 1;
                }
                if (p >= n || q >= n) continue;
                if (p > q) {
                    const int t = p;
                    p = q;
                    q = t;
                }
                T* ap = A + lda * p;
                T* aq = A + lda * q;
                double al = 0, be = 0, gr = 0, gi = 0;
                for (int r = lane; r < m; r += G) {
                    const T x = ap[r], y = aq[r];
                    al += abs2_t(x);
                    be += abs2_t(y);
                    dot_parts(x, y, gr, gi);
                }
                al = group_sum<G>(al);
                be = group_sum<G>(be);
                gr = group_sum<G>(gr);
                if (sizeof(T) == 16) gi = group_sum<G>(gi);
                if (al < negligible || be < negligible) continue;     // rounding residue: see kNegligibleColumn
                double c, sr, si, sabs, gabs;
                bool big;
                if (!rotation_fast<sizeof(T) == 16>(al, be, gr, gi, tol, c, sr, si, sabs, gabs, big)) continue;
                if (lane == 0) atomicOr(s_rot, big ? 3 : 1);
                for (int r = lane; r < m; r += G) {
                    T x = ap[r], y = aq[r];
                    rotate_pair_sg(x, y, c, sr, si);
                    ap[r] = x;
                    aq[r] = y;
                }
                T* vp = V + ldv * p;
                T* vq = V + ldv * q;
                for (int r = lane; r < n; r += G) {
                    T x = vp[r], y = vq[r];
                    rotate_pair_sg(x, y, c, sr, si);
                    vp[r] = x;
                    vq[r] = y;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        const int any = *s_rot;
        __syncthreads();
        if (!(any & 2)) break;      // nothing rotated, or only pairs already below the quadratic-phase level
    }
}


// One-sided Jacobi on every slice: the columns of A (m x n, n <= m) are rotated in place until mutually
// orthogonal; norms (n) receives the column norms = singular values.  No V accumulation: the callers
// recover the other factor with one small GEMM.  A lives in LDS for the whole iteration when it fits.
template <class T, int G, int NT>
__device__ __forceinline__ void jacobi_sweeps_nov(T* A, int lda, int m, int n, double tol, int max_sweeps,
                                                  int* s_rot, double negligible) {
    const int tid = threadIdx.x, lane = tid & (G - 1), grp = tid / G;
    constexpr int NW = NT / G;
    const int npad = n + (n & 1);
    for (int sweep = 0; sweep < max_sweeps && n > 1; ++sweep) {
        if (tid == 0) *s_rot = 0;
        __syncthreads();
        for (int round = 0; round < npad - 1; ++round) {
            for (int i = grp; i < npad / 2; i += NW) {
                int p, q;
                if (i == 0) {
                    p = npad - 1;
                    q = round;
                } else {
                    // both sums lie in [0, 2 (npad - 1)): one conditional subtraction, not a runtime modulo
                    p = round + i;
                    q = round + npad - 1 - i;
                    if (p >= npad - 1) p -= npad - 1;
                    if (q >= npad - 1) q -= npad - 1;
                }
                if (p >= n || q >= n) continue;
                T* ap = A + lda * p;
                T* aq = A + lda * q;
                double al = 0, be = 0, gr = 0, gi = 0;
                for (int r = lane; r < m; r += G) {
                    const T x = ap[r], y = aq[r];
                    al += abs2_t(x);
                    be += abs2_t(y);
                    dot_parts(x, y, gr, gi);
                }
                al = group_sum<G>(al);
                be = group_sum<G>(be);
                gr = group_sum<G>(gr);
                // a column below 1e-15 of the slice's Frobenius norm is rounding residue of a rank-deficient
                // slice: it has no direction to converge to and would keep the sweeps going (6 instead of 8.5
                // sweeps on the builder's slices); its norm is far below any truncation cutoff
                if (al < negligible || be < negligible) continue;
                double c, sn, pr, pi_unused;
                bool big;
                if (!jacobi_rotation<false>(al, be, gr, 0.0, tol, c, sn, pr, pi_unused, big)) continue;
                if (lane == 0) atomicOr(s_rot, big ? 3 : 1);
                for (int r = lane; r < m; r += G) {
                    T x = ap[r], y = aq[r];
                    rotate_pair(x, y, c, sn, pr, 0.0);
                    ap[r] = x;
                    aq[r] = y;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        const int any = *s_rot;
        __syncthreads();
        if (!(any & 2)) break;
    }
}


// ---- the store side of the fused-layout product kernels (site_apply_grouped, site_hadamard_grouped)
// result dtype of a product: real only when both operands are
template <class TW, class TA>
struct out_type {
    using type = c64;
};
template <>
struct out_type<double, double> {
    using type = double;
};

template <bool NT>
__device__ __forceinline__ void store_out(double* p, double v) {
    if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}
template <bool NT>
__device__ __forceinline__ void store_out(c64* p, c64 v) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 t = {v.re, v.im};
    if (NT) __builtin_nontemporal_store(t, reinterpret_cast<d2*>(p)); else *reinterpret_cast<d2*>(p) = t;
}

// RPL = output rows per lane: 1 for complex results (one 16-B store per element), 2 for real results (two
// adjacent rows packed into one 16-B store), so every wave-level store is 1 KiB contiguous either way.
template <class TO>
struct rows_per_lane {
    static constexpr int value = sizeof(TO) == 16 ? 1 : 2;
};

// two adjacent rows of a real result in one non-temporal 16-B store
__device__ __forceinline__ void store_pair(double* p, double v0, double v1) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 t = {v0, v1};
    __builtin_nontemporal_store(t, reinterpret_cast<d2*>(p));
}

// ---- grouped launches: one grid for all sites of a chain, the table entries carry the prefix sum of their share of it
// The index of the last of the n >= 1 entries of `tab` whose prefix field Begin (&Entry::block_begin, ...) is <= v: block -> site.
// A binary search, wave-uniform where v is.  The loop is written in its rotated form (guard + do-while) on purpose: inlined,
// that compiles to the instruction stream of the `while (lo < hi)` search spelled out in the kernel, which is what
// site_apply_grouped was measured with.
template <auto Begin, class Entry, class V>
__device__ __forceinline__ int last_entry_le(const Entry* tab, int n, V v) {
    int lo = 0, hi = n - 1;
    if (lo < hi) do {
        int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*Begin <= v) lo = mid; else hi = mid - 1;
    } while (lo < hi);
    return lo;
}

// One site of the fused-layout products (site_apply_grouped: L = the MPO site W[Dl, 2, 2, Dr]; site_hadamard_grouped: L = the
// phi site [Dl, 2, Dr]); filled by qil_product_sites (qil_apply.hip)
struct ProductSite {
    const void* L;         // left operand site
    const void* A;         // psi site  [cl, 2, cr]
    void* C;               // result    [Dl cl, 2, Dr cr]
    int Dl, Dr, cl, cr;
    long long R;           // Dl * cl   (rows)
    int row_tiles;         // ceil(R / tile rows)
    int beta_tiles;        // ceil(cr / TB)
    int b_chunks;          // ceil(Dr / NB)
    int pad;
    long long block_begin; // first workgroup of this site in the grouped grid
};

}  // namespace qil_dev
