// Pieces shared by the attention kernels (attn.hip, attn2.hip, attn_bwd_stream.hip, attn_wide.hip, attn_d256.hip): the geometry of a
// kernel configuration, the forward score pass, and every rule or operand build that more than one kernel needs -- which windows carry
// the shift mask, the clamped logit scale, the statistics operands of the K = 32 backward (attn.hip's AUG variants and
// attn_bwd_stream.hip), the L2-normalisation backward of a gradient tile.  Each is written here ONCE.
#pragma once
#include "common.h"

size_t swv2_attn_bias_range_offset(int heads, int L);       // attn.hip: the (max, min) part of a packed CPB table

namespace {

template <int LT, int DK>
struct AttnCfg {
    static constexpr int Lp = 16 * LT;
    static constexpr int DP = 16 * DK;
    static constexpr int NT = 64 * LT;          // threads per workgroup
    static constexpr int SLAB = Lp * DP;        // elements of one [Lp][DP] slab
};

// scaled / biased / masked scores of one query column (swapped layout: lane = query, acc[t][r] = key 16t + 4g + r), in
// place, log2 domain; returns the lane's partial maximum.  MASKED is the (wave-uniform) shift-mask case, instantiated
// separately so the common unmasked windows carry no select instructions; LFIX > 0 is a compile-time window area so the
// padded-key test folds away everywhere except in the last tile (the first build spent ~40 % of the forward kernel's
// instructions on these two tests).
template <int LT, bool HAS_BIAS, bool MASKED, int LFIX>
__device__ __forceinline__ float score_pass(f32x4 (&acc)[LT], const uint32_t (&biasp)[LT][2], float sc2, int Lrt, int g,
                                            int mask_thr, bool qid) {
    const int L = LFIX > 0 ? LFIX : Lrt;
    float mx = SWV2_NEG_BIG;
#pragma unroll
    for (int t = 0; t < LT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = 16 * t + 4 * g + r;
            float s;
            if (HAS_BIAS) {
                const uint32_t w = biasp[t][r >> 1];             // padded keys carry -1e30 in the bias row
                s = fmaf(acc[t][r], sc2, __uint_as_float((r & 1) ? (w & 0xffff0000u) : (w << 16)));
            } else {
                s = acc[t][r] * sc2;
                if (LFIX > 0 ? (16 * t + 16 > LFIX) : (16 * t + 16 > L)) s = (key < L) ? s : SWV2_NEG_BIG;
            }
            if (MASKED) s += ((key >= mask_thr) != qid) ? (-100.f * SWV2_LOG2E) : 0.f;
            acc[t][r] = s;
            mx = fmaxf(mx, s);
        }
    }
    return mx;
}

// ---- rules every kernel applies ------------------------------------------------------------------------------------------------
// Windows of the last window row of an image: with a shift they carry the mask (reference swinv2_global.py:403-424).  Callers write
// `(mask_thr > 0) && last_window_row(..)`: with mask_thr inside the helper the division is evaluated for unshifted blocks too.
__device__ __forceinline__ bool last_window_row(int bw, int nW, int nww, int nwh) { return ((bw % nW) / nww) == nwh - 1; }

// sigma = exp(min(tau, ln 100)): the reference's clamped logit scale.  (d tau = 0 above the clamp: the kernels test tau <= SWV2_LN100.)
__device__ __forceinline__ float clamped_logit_scale(float tau) { return __expf(fminf(tau, SWV2_LN100)); }

// ---- statistics operands of the K = 32 backward (construction: the comment above attn_bwd_kernel, attn.hip) -----------------------
// Key side, slots 16 .. 23 of a key's B-operand row: -1, -1, -1 against the three parts of lse resp. delta | -1e30 on padded keys
// (K only) | the mask term c = cmask keyed by the key's region, as hi + lo bf16 parts (k 20, 21 and k 22, 23; |error| <= 2^-17 |c|):
// one part alone is off by up to 2^-9 |c|, 0.28 in the log2 domain, which shows as soon as a masked key carries weight.
struct AugKey { uint4 k, v; };
__device__ __forceinline__ AugKey aug_key_operands(int key, int Lc, int mask_thr, float cmask) {
    const uint32_t m1 = 0xbf80u;                                       // -1
    const uint32_t padk = (key < Lc) ? 0u : (uint32_t)f2bf(-1.0e30f);
    const bool kreg = key >= mask_thr;
    const uint32_t chi = f2bf(cmask), clo = f2bf(cmask - bf2f((uint16_t)chi));
    const uint32_t mk0 = kreg ? 0u : chi, mk1 = kreg ? chi : 0u, ml0 = kreg ? 0u : clo, ml1 = kreg ? clo : 0u;
    return {make_uint4(m1 | (m1 << 16), m1 | (padk << 16), mk0 | (mk1 << 16), ml0 | (ml1 << 16)), make_uint4(m1 | (m1 << 16), m1, 0, 0)};
}

// Query side, slots 16 .. 23 of a query's rows in the Q slab (words 0 .. 3 of the result) and the dO slab (words 4 .. 7): lq = lse /
// (sigma log2 e) in three bf16 parts (1e30 on padded query rows: P = 0), a constant 1 (padded-key flag), the query's mask-region
// flags twice -- and delta in three parts.  (One register vector: a struct of two uint4 goes through memory, where the compiler
// splits and merges the words differently and the kernels' schedules change.)
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ u32x8 aug_query_row(int row, int L, int mask_thr, float lse_scaled, float delta) {
    const bool q_ok = row < L;
    const float lq = q_ok ? lse_scaled : 1.0e30f;
    uint16_t l0 = f2bf(lq);
    const float r1 = lq - bf2f(l0);
    uint16_t l1 = f2bf(r1), l2 = f2bf(r1 - bf2f(l1));
    if (!q_ok) l1 = l2 = 0;
    const uint16_t d0 = f2bf(delta);
    const float e1 = delta - bf2f(d0);
    const uint16_t d1 = f2bf(e1), d2 = f2bf(e1 - bf2f(d1));
    const uint32_t one = 0x3f80u, rqf = (row >= mask_thr) ? 0x3f80u : 0u;
    return (u32x8){l0 | ((uint32_t)l1 << 16), l2 | (one << 16), rqf | ((one - rqf) << 16), rqf | ((one - rqf) << 16),
                   d0 | ((uint32_t)d1 << 16), d2, 0, 0};
}

// delta = rowsum(dO O): the partial over one 16-byte chunk (8 channels) of the two rows
__device__ __forceinline__ float delta_partial(uint4 dO, uint4 o) {
    const uint32_t a[4] = {dO.x, dO.y, dO.z, dO.w}, b[4] = {o.x, o.y, o.z, o.w};
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        dl = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(b[e] << 16), dl);
        dl = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(b[e] & 0xffff0000u), dl);
    }
    return dl;
}

// ---- L2-normalisation backward of a 16 x 16 dQ / dK tile: x^ = r x, so dx = r (d - x^ (d . x^)), with the logit scale folded into
// rs = r sigma.  Lane (g, fr) holds channels 4g .. 4g + 3 of row fr: the row's dot product is summed over the four lane groups.
// (attn_bwd_stream.hip: both; attn_d256.hip: the second, its dot products run over 16 tiles resp. come from phase 1.  attn.hip keeps its
// own loops over the DK tiles of a row: through these functions the compiler vectorises them differently and spills more.)
__device__ __forceinline__ float l2norm_bwd_dot(f32x4 d, bf16x4 xh) {
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) dot = fmaf(d[r], bf2f(xh[r]), dot);
    return xor32_allsum(xor16_allsum(dot));
}
__device__ __forceinline__ bf16x4 l2norm_bwd_out(f32x4 d, bf16x4 xh, float rs, float dot) {
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = rs * (d[r] - bf2f(xh[r]) * dot);
    return f2bf4(v);
}

// Window area the families outside attn.hip (attn2.hip, attn_wide.hip, attn_d256.hip, attn_bwd_stream.hip) are specialised for: each has
// one instantiation for the 162-token window of the reference configuration and a run-time-L one.  THE rule: their launchers and the
// selection query (attn_select, attn.hip) both call it.
inline int attn_lfix_other(int L) { return L == 162 ? 162 : 0; }

}  // namespace
