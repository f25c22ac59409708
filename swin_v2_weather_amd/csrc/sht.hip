// Spherical-harmonic degree spectra (utils/sht.py; reference utils/losses.py:272-307, the RealSHT of GeometricH1Loss): the Legendre
// stage of the transform as a batched triangular fp32 product on the f32-input MFMA, with the degree power as its epilogue.
//
//   forward   sht_power_kernel     c[m][n][l] = sum_k T[m][l][k] X[m][n][k]  (l >= m),  n = 2 plane + (0: re, 1: im)
//                                  partial[run][plane][l] = sum_{m in run} w_m (re^2 + im^2),  w_0 = 1, else 2
//             sht_fold_kernel      power[plane][l] = sum_run partial[run][plane][l], runs in ascending order
//   backward  sht_adjoint_kernel   dX[m][n][k] = sum_{l >= m} T[m][l][k] (2 w_m g[plane][l]) c[m][n][l]
//   inverse   sht_synth_kernel     S[m][n][k] = (1 / w_k) sum_{l >= m} T[m][l][k] (f_m h[plane][l]) c[m][n][l]: the adjoint's product with
//                                  another operand scale and the row weight taken out again in the epilogue (utils/sht.py: filter, noise)
//   pairs     sht_power_kernel<true>   the forward on planes interleaved as pairs (a_p, b_p): besides the two auto spectra the cross
//                                  spectrum  partial[run][2 pairs + p][l] = sum_{m in run} w_m (re_a re_b + im_a im_b)  (utils/sht.py: cross_power)
//             sht_cross_adjoint_kernel   dX[m][n][k] = sum_{l >= m} T[m][l][k] ((2 w_m g_self[p][l]) c[m][n][l] + (w_m g_ab[p][l]) c[m][n ^ 2][l])
//   both      sht_repack_kernel    rfft's layout [plane][k][m][re, im] <-> the operand layout [m][n][k], times 2 pi
//
// Layouts.  T [mmax][lmax][nlat] dense (entries l < m are zero and never read); X and dX [mmax][2 planes][nlat]; the coefficients
// [mmax][2 planes][lmax], written for l >= m only (the adjoint reads nothing else).  Every operand of both products is contiguous along
// the index a wave's lanes run over when they write it: the outputs leave as 128-byte rows.
//
// One tile routine (tile_product) serves both: a workgroup of 4 waves forms a [64 n] x [128 o] tile of  D[n][o] = sum_r A[n][r] B[r][o]
// with v_mfma_f32_32x32x2_f32, wave w owning the n half (w & 1) and the o half (w >> 1) as two 32 x 32 accumulators that share the A
// operand.  Both operands are staged in LDS as [r][out] with a pitch of out + 2 floats; the MFMA's two k slots take rows r and r + 16
// of a 32-deep stage, which are 16 * pitch = 32 (mod 64) banks apart, so the 64 lanes of an operand read hit 64 different banks.  An
// operand that is contiguous along r in memory (T and X in the forward, the coefficients in the adjoint) is transposed on its way in:
// a wave writes 32 r x 2 out, banks 2 r + out, again all different.  Loads are single floats with a predicate (odd nlat, odd lmax: no
// alignment to rely on); the next stage's loads are in flight while the current one is multiplied.
//
// Triangle.  In the forward a 32-row block of l that lies wholly below m is skipped by its wave (no MFMA) and its table rows are not
// loaded; a workgroup whose 128 rows lie below the first m of its run returns at once.  In the adjoint the reduction runs over
// [m, lmax) only.  So the products skipped are those of whole 32-blocks; inside a straddling block the rows l < m meet zeros.
//
// Sums.  No atomics: a workgroup adds the m of its run (SHT_MRUN adjacent m, ascending) into its own registers and stores one partial
// per (run, plane, l); sht_fold_kernel adds the runs  r <= l / SHT_MRUN  in ascending order.  Two runs on the same input agree bit for
// bit.  The chain of one coefficient is the MFMA's k-ordered fp32 fma chain over the stage rows in the order 0, 16, 1, 17, ...
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int SHT_MRUN = 8;            // adjacent m per forward workgroup
constexpr int SHT_TN = 64;             // tile extent along n (the A side)
constexpr int SHT_TO = 128;            // tile extent along o (the B side): l in the forward, k in the adjoint
constexpr int SHT_RT = 32;             // reduction depth of one stage
constexpr int SHT_PA = SHT_TN + 2, SHT_PB = SHT_TO + 2;
static_assert((16 * SHT_PA) % 64 == 32 && (16 * SHT_PB) % 64 == 32, "rows r and r + 16 must be 32 banks apart");

struct NoScale {
    __device__ __forceinline__ float operator()(float v, int, int) const { return v; }
};

// the adjoint's A operand: c[n][l] times 2 w_m g[plane][l]
struct GradScale {
    const float* g;          // [planes][lmax]
    int lmax;
    float w2;
    __device__ __forceinline__ float operator()(float v, int n, int l) const { return (w2 * g[(size_t)(n >> 1) * lmax + l]) * v; }
};

// the synthesis' A operand: c[n][l] times f_m h[plane][l] (hs = 0: one response for all planes; without H: h = 1)
template <bool H>
struct SynthScale {
    const float* h;          // [planes][lmax] or [lmax]
    int hs;
    float f;
    bool real;               // this m's imaginary rows (n odd) count as zeros
    __device__ __forceinline__ float operator()(float v, int n, int l) const {
        const float s = H ? f * h[(size_t)(n >> 1) * hs + l] : f;          // (loaded under the caller's predicate only: the select comes last)
        return real && (n & 1) ? 0.f : s * v;
    }
};

// the cross adjoint's A operand.  Column n = 4 p + (0: re a, 1: im a, 2: re b, 3: im b) of pair p has its partner (the same part of the
// other plane) at n ^ 2, and  d/dc[n] of  g_aa P_aa + g_bb P_bb + g_ab C_ab  is  2 w_m g_self c[n] + w_m g_ab c[n ^ 2],  g_self = g_aa for the
// a columns (n & 2 == 0), g_bb for the b columns.  Roundings, in this order: s = w2 g_self and t = w1 g_ab are exact (w2 = 2 w_m and
// w1 = w_m are powers of two); t c[n ^ 2] is rounded once; fmaf(s, c[n], that) once.  The partner is read here, under the caller's predicate
// (n < N implies n ^ 2 < N because N is a multiple of 4; l is in [m, lmax), the rows that were written).
struct CrossScale {
    const float* g;          // [3][pairs][lmax]: g_aa, g_bb, g_ab
    const float* cm;         // this m's coefficients [4 pairs][lmax]
    int lmax, pairs;
    float w2, w1;
    __device__ __forceinline__ float operator()(float v, int n, int l) const {
        const int p = n >> 2;
        const float s = w2 * g[((size_t)((n >> 1) & 1) * pairs + p) * lmax + l], t = w1 * g[((size_t)2 * pairs + p) * lmax + l];
        return fmaf(s, v, t * cm[(size_t)(n ^ 2) * lmax + l]);
    }
};

// One operand stage, global -> registers: OUT x SHT_RT elements, element (o, r) at src[(o0 + o) * ld + r] (TR: contiguous along r) or
// src[r * ld + o0 + o] (contiguous along o); zero outside o in [o_lo, o_hi), r in [r_lo, r_hi).  r0 is the stage's first r.
template <int OUT, bool TR, class F>
__device__ __forceinline__ void stage_load(float (&v)[OUT * SHT_RT / 256], const float* __restrict__ src, int ld, int o0, int o_lo, int o_hi,
                                           int r0, int r_lo, int r_hi, F f) {
    // element e of a thread: (o, r) = (ot + 8 e, rt) (TR) or (ot, rt + (256 / OUT) e); the thread's own offset is one register, what changes
    // with e and with the stage is uniform and goes into the scalar base of the load.  Offsets < 2^31: checked by the host.
    constexpr int RSTEP = 256 / OUT;
    const int ot = o0 + (TR ? (int)threadIdx.x / SHT_RT : (int)threadIdx.x % OUT), rt = TR ? (int)threadIdx.x % SHT_RT : (int)threadIdx.x / OUT;
    const uint32_t voff = TR ? (uint32_t)(ot * ld + rt) : (uint32_t)(rt * ld + ot);
#pragma unroll
    for (int e = 0; e < OUT * SHT_RT / 256; ++e) {
        const int o = TR ? ot + 8 * e : ot, r = r0 + (TR ? rt : rt + RSTEP * e);
        const float* sp = src + (TR ? (size_t)(uint32_t)(8 * e * ld + r0) : (size_t)(uint32_t)((r0 + RSTEP * e) * ld));
        float x = 0.f;
        if (o >= o_lo && o < o_hi && r >= r_lo && r < r_hi) x = f(sp[voff], o, r);
        v[e] = x;
    }
}

template <int OUT, bool TR>
__device__ __forceinline__ void stage_store(const float (&v)[OUT * SHT_RT / 256], float* __restrict__ lds) {
#pragma unroll
    for (int e = 0; e < OUT * SHT_RT / 256; ++e) {
        const int idx = e * 256 + threadIdx.x;
        const int r = TR ? idx % SHT_RT : idx / OUT, o = TR ? idx / SHT_RT : idx % OUT;
        lds[r * (OUT + 2) + o] = v[e];
    }
}

// acc[j][..] += sum over r in [r_lo, r_hi) of A[n][r] B[r][o] for the wave's 32 n and its two 32-blocks of o (use[j]: wave-uniform).
// Result map of a 32 x 32 accumulator: n = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), o = lane & 31.
template <bool TRA, bool TRB, class FA>
__device__ __forceinline__ void tile_product(f32x16 (&acc)[2], const bool (&use)[2], const float* __restrict__ A, int lda, int n0, int n_hi,
                                             FA fa, const float* __restrict__ B, int ldb, int o0, int o_lo, int o_hi, int r_lo, int r_hi,
                                             float* __restrict__ As, float* __restrict__ Bs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int an = (wave & 1) * 32 + (lane & 31), bo = (wave >> 1) * 64 + (lane & 31), rh = (lane >> 5) * 16;
    float va[SHT_TN * SHT_RT / 256], vb[SHT_TO * SHT_RT / 256];
    stage_load<SHT_TN, TRA>(va, A, lda, n0, 0, n_hi, r_lo, r_lo, r_hi, fa);
    stage_load<SHT_TO, TRB>(vb, B, ldb, o0, o_lo, o_hi, r_lo, r_lo, r_hi, NoScale());
    for (int r0 = r_lo; r0 < r_hi; r0 += SHT_RT) {
        __syncthreads();                                       // the previous stage has been multiplied
        stage_store<SHT_TN, TRA>(va, As);
        stage_store<SHT_TO, TRB>(vb, Bs);
        __syncthreads();
        if (r0 + SHT_RT < r_hi) {
            stage_load<SHT_TN, TRA>(va, A, lda, n0, 0, n_hi, r0 + SHT_RT, r_lo, r_hi, fa);
            stage_load<SHT_TO, TRB>(vb, B, ldb, o0, o_lo, o_hi, r0 + SHT_RT, r_lo, r_hi, NoScale());
        }
        // (the wave-uniform choice outside the unrolled loop: a branch around every MFMA keeps the compiler from running the LDS reads ahead)
        if (use[0] && use[1]) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float a = As[(kk + rh) * SHT_PA + an];
                const float b0 = Bs[(kk + rh) * SHT_PB + bo], b1 = Bs[(kk + rh) * SHT_PB + bo + 32];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
            }
        } else if (use[0]) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + rh) * SHT_PA + an], Bs[(kk + rh) * SHT_PB + bo], acc[0], 0, 0, 0);
        } else if (use[1]) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + rh) * SHT_PA + an], Bs[(kk + rh) * SHT_PB + bo + 32], acc[1], 0, 0, 0);
        }
    }
}

// grid (l tiles of 128, n tiles of 64, runs of SHT_MRUN m).  CROSS: the planes are pairs (a_p, b_p) = planes (2 p, 2 p + 1); an accumulator's
// registers 4 g .. 4 g + 3 of a lane are re a, im a, re b, im b of one pair at one (m, l), so the cross term needs no lane movement.  The auto
// terms are formed exactly as without CROSS (the same bits as the plain forward on the same planes); the partials then lie as
// ws[run][3 pairs][lmax]: rows p of P_aa, pairs + p of P_bb, 2 pairs + p of C_ab -- sht_fold_kernel with 3 pairs "planes" leaves [3][pairs][lmax].
template <bool CROSS>
__global__ __launch_bounds__(256, 2) void sht_power_kernel(const float* __restrict__ T, const float* __restrict__ X, float* __restrict__ ws,
                                                        float* __restrict__ coef, int planes, int nlat, int lmax, int mmax) {
    __shared__ float As[SHT_RT * SHT_PA], Bs[SHT_RT * SHT_PB];
    const int l0 = blockIdx.x * SHT_TO, n0 = blockIdx.y * SHT_TN, m0 = blockIdx.z * SHT_MRUN, N = 2 * planes;
    const int m_end = min(min(m0 + SHT_MRUN, mmax), min(lmax, l0 + SHT_TO));          // m <= l needs m < l0 + 128
    if (m0 >= m_end) return;                                                           // (uniform) nothing of this run reaches these rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lw = l0 + (wave >> 1) * 64, nw = n0 + (wave & 1) * 32 + 4 * (lane >> 5);
    float pw[2][8], cx[2][CROSS ? 4 : 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int q = 0; q < 8; ++q) pw[j][q] = 0.f;
#pragma unroll
        for (int q = 0; q < (CROSS ? 4 : 1); ++q) cx[j][q] = 0.f;
    }
    for (int m = m0; m < m_end; ++m) {
        f32x16 acc[2];
        bool use[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            use[j] = lw + 32 * j + 31 >= m && lw + 32 * j < lmax;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        }
        tile_product<true, true>(acc, use, X + (size_t)m * N * nlat, nlat, n0, N, NoScale(), T + (size_t)m * lmax * nlat, nlat,
                                 l0, m, lmax, 0, nlat, As, Bs);
        const float wm = m == 0 ? 1.f : 2.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!use[j]) continue;
            const int l = lw + 32 * j + (lane & 31);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float re = acc[j][2 * q], im = acc[j][2 * q + 1];
                pw[j][q] = fmaf(wm, fmaf(im, im, re * re), pw[j][q]);
            }
            if (CROSS) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    cx[j][q] = fmaf(wm, fmaf(acc[j][4 * q + 1], acc[j][4 * q + 3], acc[j][4 * q] * acc[j][4 * q + 2]), cx[j][q]);
            }
            if (coef && l >= m && l < lmax) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int n = nw + (q & 3) + 8 * (q >> 2);
                    if (n < N) coef[((size_t)m * N + n) * lmax + l] = acc[j][q];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int l = lw + 32 * j + (lane & 31);
        if (l >= lmax) continue;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = nw + 2 * (q & 1) + 8 * (q >> 1);                             // the even (re) row of the pair
            if (!CROSS) {
                if (n < N) ws[((size_t)blockIdx.z * planes + (n >> 1)) * lmax + l] = pw[j][q];
            } else if (n < N) ws[((size_t)blockIdx.z * 3 * (planes >> 1) + (size_t)(q & 1) * (planes >> 1) + (n >> 2)) * lmax + l] = pw[j][q];      // q & 1: a or b
        }
        if (CROSS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = nw + 8 * q;
                if (n < N) ws[((size_t)blockIdx.z * 3 * (planes >> 1) + (size_t)2 * (planes >> 1) + (n >> 2)) * lmax + l] = cx[j][q];
            }
        }
    }
}

__global__ __launch_bounds__(256) void sht_fold_kernel(const float* __restrict__ ws, float* __restrict__ power, int planes, int lmax, int mtop) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)planes * lmax;
    if (i >= total) return;
    const int l = (int)(i % lmax);
    const int runs = min(l, mtop - 1) / SHT_MRUN + 1;          // the runs whose first m is <= l (and below min(mmax, lmax))
    float s = 0.f;
    for (int r = 0; r < runs; ++r) s += ws[(size_t)r * total + i];
    power[i] = s;
}

// The product both ways back share: out[m][n][k] = (RW ? rw[k] : 1) sum_{l >= m} T[m][l][k] fa(c[m][n][l]).  grid (k tiles of 128, n tiles of 64, mmax)
template <bool RW, class FA>
__device__ __forceinline__ void back_tile(const float* __restrict__ T, const float* __restrict__ coef, FA fa, const float* __restrict__ rw,
                                          float* __restrict__ out, int planes, int nlat, int lmax, float* __restrict__ As, float* __restrict__ Bs) {
    const int k0 = blockIdx.x * SHT_TO, n0 = blockIdx.y * SHT_TN, m = blockIdx.z, N = 2 * planes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kw = k0 + (wave >> 1) * 64, nw = n0 + (wave & 1) * 32 + 4 * (lane >> 5);
    f32x16 acc[2];
    bool use[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        use[j] = kw + 32 * j < nlat;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    }
    if (m < lmax)                                              // (uniform) else no degree has this m: the result is zero
        tile_product<true, false>(acc, use, coef + (size_t)m * N * lmax, lmax, n0, N, fa, T + (size_t)m * lmax * nlat, nlat, k0, 0, nlat, m, lmax,
                                  As, Bs);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = kw + 32 * j + (lane & 31);
        if (k >= nlat) continue;
        const float r = RW ? rw[k] : 1.f;                      // one load per accumulator column
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int n = nw + (q & 3) + 8 * (q >> 2);
            if (n < N) out[((size_t)m * N + n) * nlat + k] = RW ? r * acc[j][q] : acc[j][q];
        }
    }
}

__global__ __launch_bounds__(256, 2) void sht_adjoint_kernel(const float* __restrict__ T, const float* __restrict__ coef, const float* __restrict__ g,
                                                          float* __restrict__ dX, int planes, int nlat, int lmax) {
    __shared__ float As[SHT_RT * SHT_PA], Bs[SHT_RT * SHT_PB];
    back_tile<false>(T, coef, GradScale{g, lmax, blockIdx.z == 0 ? 2.f : 4.f}, nullptr, dX, planes, nlat, lmax, As, Bs);
}

__global__ __launch_bounds__(256, 2) void sht_cross_adjoint_kernel(const float* __restrict__ T, const float* __restrict__ coef,
                                                                const float* __restrict__ g, float* __restrict__ dX, int pairs, int nlat, int lmax) {
    __shared__ float As[SHT_RT * SHT_PA], Bs[SHT_RT * SHT_PB];
    const bool m0 = blockIdx.z == 0;
    back_tile<false>(T, coef, CrossScale{g, coef + (size_t)blockIdx.z * 4 * pairs * lmax, lmax, pairs, m0 ? 2.f : 4.f, m0 ? 1.f : 2.f}, nullptr, dX,
                     2 * pairs, nlat, lmax, As, Bs);
}

// S[m][n][k] = rw[k] sum_{l >= m} T[m][l][k] (f_m h[plane][l]) c[m][n][l]; the imaginary rows of m = 0 and of m = m_nyq (nlon / 2 for an even
// nlon, else -1) are not read and leave as zeros
template <bool H>
__global__ __launch_bounds__(256, 2) void sht_synth_kernel(const float* __restrict__ T, const float* __restrict__ rw, const float* __restrict__ coef,
                                                        const float* __restrict__ h, int hs, float f0, float fm, int m_nyq, float* __restrict__ S,
                                                        int planes, int nlat, int lmax) {
    __shared__ float As[SHT_RT * SHT_PA], Bs[SHT_RT * SHT_PB];
    const int m = blockIdx.z;
    back_tile<true>(T, coef, SynthScale<H>{h, hs, m == 0 ? f0 : fm, m == 0 || m == m_nyq}, rw, S, planes, nlat, lmax, As, Bs);
}

// The longitude transform as torch.fft.rfft leaves it, F [planes][nlat][mmax][2] (m, then re / im, innermost), <-> the operand layout:
//   forward   X[m][2 p + ri][k] = scale F[p][k][m][ri]          backward   dF[p][k][m][ri] = scale dX[m][2 p + ri][k]
// grid (k tiles of 32, m tiles of 32, planes): a 32 k x 64 (m, ri) tile through LDS (pitch 65), read and written as contiguous runs of
// 256 bytes (F side) and 128 bytes (X side).
template <bool BACK>
__global__ __launch_bounds__(256) void sht_repack_kernel(const float* __restrict__ src, float* __restrict__ dst, int planes, int nlat, int mmax,
                                                         float scale) {
    __shared__ float t[32][65];
    const int k0 = blockIdx.x * 32, m0 = blockIdx.y * 32, p = blockIdx.z, N = 2 * planes;
    const int fc = threadIdx.x & 63, fk = threadIdx.x >> 6;          // F side: column (m, ri) and row k (+ 4 per pass)
    const int xk = threadIdx.x & 31, xc = threadIdx.x >> 5;          // X side: k and column (+ 8 per pass)
    const size_t fbase = ((size_t)p * nlat) * mmax * 2;
    if (!BACK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + fk + 4 * i, m = m0 + (fc >> 1);
            if (k < nlat && m < mmax) t[fk + 4 * i][fc] = src[fbase + ((size_t)k * mmax + m) * 2 + (fc & 1)];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = xc + 8 * i, k = k0 + xk, m = m0 + (c >> 1);
            if (k < nlat && m < mmax) t[xk][c] = src[((size_t)m * N + 2 * p + (c & 1)) * nlat + k];
        }
    }
    __syncthreads();
    if (!BACK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = xc + 8 * i, k = k0 + xk, m = m0 + (c >> 1);
            if (k < nlat && m < mmax) dst[((size_t)m * N + 2 * p + (c & 1)) * nlat + k] = scale * t[xk][c];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + fk + 4 * i, m = m0 + (fc >> 1);
            if (k < nlat && m < mmax) dst[fbase + ((size_t)k * mmax + m) * 2 + (fc & 1)] = scale * t[fk + 4 * i][fc];
        }
    }
}

inline bool sht_shape_ok(int planes, int nlat, int lmax, int mmax) {
    // (one m's slice of every operand is indexed with 32 bits)
    return planes > 0 && nlat > 0 && lmax > 0 && mmax > 0 && planes <= (1 << 20) && nlat <= (1 << 15) && lmax <= (1 << 15) && mmax <= 65535 &&
           2L * planes * (nlat > lmax ? nlat : lmax) < (1L << 31) && (long)lmax * nlat < (1L << 31);
}

}  // namespace

extern "C" size_t swv2_sht_ws_bytes(int planes, int lmax, int mmax) {
    if (planes <= 0 || lmax <= 0 || mmax <= 0) return 0;
    return (size_t)cdiv(mmax < lmax ? mmax : lmax, SHT_MRUN) * planes * lmax * sizeof(float);
}

extern "C" int swv2_sht_power(const float* table, const float* X, float* power, float* coeffs, int planes, int nlat, int lmax, int mmax,
                              void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(table && X && power && ws, "sht_power: null pointer");
    SWV2_CHECK_ARG(sht_shape_ok(planes, nlat, lmax, mmax), "sht_power: bad shape (planes, nlat, lmax, mmax > 0; planes <= 2^20, nlat, lmax <= 2^15, mmax < 2^16)");
    SWV2_CHECK_ARG(cdiv(2L * planes, SHT_TN) <= 65535, "sht_power: too many planes for one launch");
    SWV2_CHECK_ARG(ws_bytes >= swv2_sht_ws_bytes(planes, lmax, mmax), "sht_power: workspace too small (swv2_sht_ws_bytes)");
    const int mtop = mmax < lmax ? mmax : lmax;
    hipLaunchKernelGGL(sht_power_kernel<false>, dim3(cdiv(lmax, SHT_TO), cdiv(2L * planes, SHT_TN), cdiv(mtop, SHT_MRUN)), dim3(256), 0, (hipStream_t)stream,
                       table, X, (float*)ws, coeffs, planes, nlat, lmax, mmax);
    SWV2_CHECK_LAUNCH("swv2_sht_power");
    hipLaunchKernelGGL(sht_fold_kernel, dim3(cdiv((long)planes * lmax, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, power, planes,
                       lmax, mtop);
    SWV2_CHECK_LAUNCH("swv2_sht_power (fold)");
    return SWV2_OK;
}

extern "C" size_t swv2_sht_cross_ws_bytes(int pairs, int lmax, int mmax) {
    if (pairs <= 0 || lmax <= 0 || mmax <= 0) return 0;
    return (size_t)cdiv(mmax < lmax ? mmax : lmax, SHT_MRUN) * 3 * pairs * lmax * sizeof(float);
}

extern "C" int swv2_sht_cross_power(const float* table, const float* X, float* spectra, float* coeffs, int pairs, int nlat, int lmax, int mmax,
                                    void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(table && X && spectra && ws, "sht_cross_power: null pointer");
    SWV2_CHECK_ARG(pairs > 0 && pairs <= 32767, "sht_cross_power: pairs outside 1 .. 32767");
    SWV2_CHECK_ARG(sht_shape_ok(2 * pairs, nlat, lmax, mmax), "sht_cross_power: bad shape (nlat, lmax, mmax > 0; nlat, lmax <= 2^15, mmax < 2^16; one m's slice < 2^31 elements)");
    SWV2_CHECK_ARG(ws_bytes >= swv2_sht_cross_ws_bytes(pairs, lmax, mmax), "sht_cross_power: workspace too small (swv2_sht_cross_ws_bytes)");
    const int mtop = mmax < lmax ? mmax : lmax;
    hipLaunchKernelGGL(sht_power_kernel<true>, dim3(cdiv(lmax, SHT_TO), cdiv(4L * pairs, SHT_TN), cdiv(mtop, SHT_MRUN)), dim3(256), 0, (hipStream_t)stream,
                       table, X, (float*)ws, coeffs, 2 * pairs, nlat, lmax, mmax);
    SWV2_CHECK_LAUNCH("swv2_sht_cross_power");
    hipLaunchKernelGGL(sht_fold_kernel, dim3(cdiv(3L * pairs * lmax, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, spectra, 3 * pairs,
                       lmax, mtop);
    SWV2_CHECK_LAUNCH("swv2_sht_cross_power (fold)");
    return SWV2_OK;
}

extern "C" int swv2_sht_cross_adjoint(const float* table, const float* coeffs, const float* gspectra, float* dX, int pairs, int nlat, int lmax, int mmax,
                                      void* stream) {
    SWV2_CHECK_ARG(table && coeffs && gspectra && dX, "sht_cross_adjoint: null pointer");
    SWV2_CHECK_ARG(pairs > 0 && pairs <= 32767, "sht_cross_adjoint: pairs outside 1 .. 32767");
    SWV2_CHECK_ARG(sht_shape_ok(2 * pairs, nlat, lmax, mmax), "sht_cross_adjoint: bad shape (nlat, lmax, mmax > 0; nlat, lmax <= 2^15, mmax < 2^16; one m's slice < 2^31 elements)");
    hipLaunchKernelGGL(sht_cross_adjoint_kernel, dim3(cdiv(nlat, SHT_TO), cdiv(4L * pairs, SHT_TN), mmax), dim3(256), 0, (hipStream_t)stream, table, coeffs,
                       gspectra, dX, pairs, nlat, lmax);
    SWV2_CHECK_LAUNCH("swv2_sht_cross_adjoint");
    return SWV2_OK;
}

extern "C" int swv2_sht_adjoint(const float* table, const float* coeffs, const float* gpower, float* dX, int planes, int nlat, int lmax, int mmax,
                                void* stream) {
    SWV2_CHECK_ARG(table && coeffs && gpower && dX, "sht_adjoint: null pointer");
    SWV2_CHECK_ARG(sht_shape_ok(planes, nlat, lmax, mmax), "sht_adjoint: bad shape (planes, nlat, lmax, mmax > 0; planes <= 2^20, nlat, lmax <= 2^15, mmax < 2^16)");
    SWV2_CHECK_ARG(cdiv(2L * planes, SHT_TN) <= 65535, "sht_adjoint: too many planes for one launch");
    hipLaunchKernelGGL(sht_adjoint_kernel, dim3(cdiv(nlat, SHT_TO), cdiv(2L * planes, SHT_TN), mmax), dim3(256), 0, (hipStream_t)stream, table, coeffs,
                       gpower, dX, planes, nlat, lmax);
    SWV2_CHECK_LAUNCH("swv2_sht_adjoint");
    return SWV2_OK;
}

extern "C" int swv2_sht_synth(const float* table, const float* rweights, const float* coeffs, const float* response, int response_stride,
                              float scale_m0, float scale_m, float* S, int planes, int nlat, int lmax, int mmax, int nlon, void* stream) {
    SWV2_CHECK_ARG(table && rweights && coeffs && S, "sht_synth: null pointer");
    SWV2_CHECK_ARG(sht_shape_ok(planes, nlat, lmax, mmax), "sht_synth: bad shape (planes, nlat, lmax, mmax > 0; planes <= 2^20, nlat, lmax <= 2^15, mmax < 2^16)");
    SWV2_CHECK_ARG(cdiv(2L * planes, SHT_TN) <= 65535, "sht_synth: too many planes for one launch");
    SWV2_CHECK_ARG(response_stride == 0 || response_stride == lmax, "sht_synth: response_stride is 0 (one response) or lmax (one per plane)");
    SWV2_CHECK_ARG(nlon >= 1, "sht_synth: nlon < 1");
    const dim3 grid(cdiv(nlat, SHT_TO), cdiv(2L * planes, SHT_TN), mmax);
    const int m_nyq = nlon % 2 == 0 ? nlon / 2 : -1;
    if (response)
        hipLaunchKernelGGL(sht_synth_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, table, rweights, coeffs, response, response_stride,
                           scale_m0, scale_m, m_nyq, S, planes, nlat, lmax);
    else
        hipLaunchKernelGGL(sht_synth_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, table, rweights, coeffs, response, response_stride,
                           scale_m0, scale_m, m_nyq, S, planes, nlat, lmax);
    SWV2_CHECK_LAUNCH("swv2_sht_synth");
    return SWV2_OK;
}

extern "C" int swv2_sht_repack(const float* src, float* dst, int planes, int nlat, int mmax, float scale, int backward, void* stream) {
    SWV2_CHECK_ARG(src && dst, "sht_repack: null pointer");
    SWV2_CHECK_ARG(planes > 0 && nlat > 0 && mmax > 0 && planes <= 65535 && cdiv(mmax, 32) <= 65535, "sht_repack: bad shape (planes, nlat, mmax > 0; planes < 2^16)");
    const dim3 grid(cdiv(nlat, 32), cdiv(mmax, 32), planes);
    if (backward)
        hipLaunchKernelGGL(sht_repack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, planes, nlat, mmax, scale);
    else
        hipLaunchKernelGGL(sht_repack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, planes, nlat, mmax, scale);
    SWV2_CHECK_LAUNCH("swv2_sht_repack");
    return SWV2_OK;
}
