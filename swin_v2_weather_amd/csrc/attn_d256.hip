// Window attention for 256-channel heads (embed 2048 / 8 heads, the reference's `..._e2048_...` yaml entry) in the 176-row window
// layout (window areas 65 .. 176), no CPB bias.  Same semantics, data layout and lse convention as attn_wide.hip; what differs is
// that no operand of a (window, head) fits in LDS beside another at this width: the K and V slabs of a 176-row window are 90 KB each.
//
// forward (attn_fwd_d256_kernel): wave = query tile, swapped product S^T = K Q^T (a lane owns one query column), row-maximum softmax
//   exactly as attn_fwd_wide_kernel.  The whole K slab is staged (176 x 272 bf16 = 94 KB), the scores of the wave's 16 queries stay
//   in registers through the softmax, then the V slab is staged over K and O^T = V^T P^T runs over pairs of key tiles.
//   Q fragments come from global memory straight into the MFMA B operands.
// backward (attn_bwd_d256_kernel): wave = key tile in phase 1, wave = query tile in phase 2 (as attn_bwd_wide_kernel), with the
//   channels walked in four 64-column chunks:
//   * S = Q K^T and dP = dO V^T are summed over the chunks in registers (11 + 11 accumulators per lane; the Q / dO chunk staged
//     in LDS, the K / V chunk of the wave's key tile loaded into registers); delta = rowsum(dO O) is summed over the same chunks;
//   * P and dS are formed once, kept as bf16 MFMA operands in registers (P, dS) and in the LDS image [key][q] (dS, phase 2);
//   * dV^T += dO^T P, dK^T += Q^T dS per chunk (chunk order 3, 2, 1, 0: the last staged chunk is reused), each chunk's dK / dV
//     written at once.  The L2-normalisation backward needs sum_d dK[k][d] k^[k][d] = sum_q dS[q][k] cos[q][k] before the first
//     chunk is final: it is taken from the fp32 dS and score accumulators (no pass over all 256 columns of dK);
//   * phase 2: dQ^T = sum_t K_t^T dS_t^T with the K chunks staged in turn, all 256 columns accumulated (64 registers), then
//     the normalisation backward of dQ.
//   LDS 113 KB, one workgroup of 11 waves per CU.  d(qkv) is deterministic; d logit_scale is one float atomic per workgroup (the
//   caller zeroes it), so its last bits depend on the order in which the workgroups finish.
#include "attn_common.h"

namespace {

constexpr int D256_LT = 11, D256_LP = 16 * D256_LT, D256_DP = 256, D256_NT = 64 * D256_LT;

template <int LFIX>
__global__ __launch_bounds__(D256_NT) void attn_fwd_d256_kernel(
    const uint16_t* __restrict__ qkvh, const float* __restrict__ logit_scale, uint16_t* __restrict__ oh, float* __restrict__ lse,
    int Bw, int h, int L, int nW, int nww, int nwh, int mask_thr) {
    constexpr int LT = D256_LT, Lp = D256_LP, DP = D256_DP, SLAB = Lp * DP, NT = D256_NT;
    constexpr int QP = DP + 16;                              // row pitch (elements) of the staged slab: 544 bytes
    constexpr int KS = DP / 32, DT = DP / 16;
    static_assert(Lp * QP * 2 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) uint16_t KV[Lp * QP];       // K, then V
    const int hd = blockIdx.y;
    const float sc2 = clamped_logit_scale(logit_scale[hd]) * SWV2_LOG2E;
    // staging map: 32 threads per row (one 16-byte chunk each), 22 rows per pass, 8 passes
    constexpr int TPR = DP / 8, RPP = NT / TPR, PASSES = Lp / RPP;
    static_assert(Lp % RPP == 0, "staging map");
    const uint32_t nobias[LT][2] = {};

    for (int bw = blockIdx.x; bw < Bw; bw += gridDim.x) {
        int tid = threadIdx.x;                                // lane-derived offsets recomputed per window (see attn_bwd_d256_kernel)
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, qt = tid >> 6;
        const int fr = lane & 15, g = lane >> 4;
        const int q = 16 * qt + fr;
        const int srow = tid / TPR, scc = tid % TPR;
        auto stage = [&](size_t src) {
            bf16x8 r[PASSES];                                 // (a uint4 array stays an alloca: scratch)
#pragma unroll
            for (int p = 0; p < PASSES; ++p) r[p] = *(const bf16x8*)(qkvh + src + (size_t)(srow + RPP * p) * DP + scc * 8);
#pragma unroll
            for (int p = 0; p < PASSES; ++p) *(bf16x8*)(KV + (srow + RPP * p) * QP + scc * 8) = r[p];
        };
        const size_t slab0 = ((size_t)bw * h + hd) * 3 * SLAB;
        f32x4 acc[LT];
        {
            bf16x8 qf[KS];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) qf[kk] = *(const bf16x8*)(qkvh + slab0 + (size_t)q * DP + 32 * kk + 8 * g);
            stage(slab0 + SLAB);
            __syncthreads();
            // S^T tiles: rows = keys 16 t + 4 g + r, column = query fr
#pragma unroll
            for (int t = 0; t < LT; ++t) {
                acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const bf16x8 kf = *(const bf16x8*)(KV + (16 * t + fr) * QP + 32 * kk + 8 * g);
                    acc[t] = mfma32(kf, qf[kk], acc[t]);
                }
            }
        }
        __syncthreads();                                      // every wave is done with K: V goes over it
        stage(slab0 + 2 * SLAB);

        const bool do_mask = (mask_thr > 0) && last_window_row(bw, nW, nww, nwh);
        float mx, sum = 0.f;
        if (!do_mask) {          // sigma > 0 commutes with the maximum: the scale is folded into the exponent's fma (attn_fwd_kernel)
            const int Lc = LFIX > 0 ? LFIX : L;
            mx = SWV2_NEG_BIG;
#pragma unroll
            for (int t = 0; t < LT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (16 * t + 16 > Lc) acc[t][r] = (16 * t + 4 * g + r < Lc) ? acc[t][r] : SWV2_NEG_BIG;
                    mx = fmaxf(mx, acc[t][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            mx *= sc2;
#pragma unroll
            for (int t = 0; t < LT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(acc[t][r], sc2, -mx));
                    acc[t][r] = p;
                    sum += p;
                }
        } else {
            mx = score_pass<LT, false, true, LFIX>(acc, nobias, sc2, L, g, mask_thr, q >= mask_thr);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
#pragma unroll
            for (int t = 0; t < LT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(acc[t][r] - mx);
                    acc[t][r] = p;
                    sum += p;
                }
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        __syncthreads();                                      // V staged

        // O^T[d][q] = sum_keys V^T[d][key] P^T[key][q]: key tiles in pairs (K = 32), the odd last tile as a K = 16 product
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t + 1 < LT; t += 2) {
            const bf16x8 pb = __builtin_shufflevector(f2bf4(acc[t]), f2bf4(acc[t + 1]), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x4 v0 = lds_tr_read(KV + (16 * t + 4 * g + (fr >> 2)) * QP + 16 * dt + (fr & 3) * 4);
                const bf16x4 v1 = lds_tr_read(KV + (16 * (t + 1) + 4 * g + (fr >> 2)) * QP + 16 * dt + (fr & 3) * 4);
                o[dt] = mfma32(__builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7), pb, o[dt]);
            }
        }
        if (LT & 1) {
            const bf16x4 pb = f2bf4(acc[LT - 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x4 vf = lds_tr_read(KV + (16 * (LT - 1) + 4 * g + (fr >> 2)) * QP + 16 * dt + (fr & 3) * 4);
                const f32x4 tail = mfma16(vf, pb, (f32x4){0.f, 0.f, 0.f, 0.f});
                o[dt] += tail;
            }
        }
        const float inv = (q < L) ? 1.f / sum : 0.f;          // padded query rows: zeros
        uint16_t* orow = oh + ((size_t)bw * h + hd) * SLAB + (size_t)q * DP;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            f32x4 v = o[dt];
            v[0] *= inv; v[1] *= inv; v[2] *= inv; v[3] *= inv;
            *(bf16x4*)(orow + 16 * dt + 4 * g) = f2bf4(v);
        }
        if (g == 0) lse[((size_t)bw * h + hd) * Lp + q] = (q < L) ? mx + __log2f(sum) : 0.f;
        __syncthreads();                                      // the next window's staging overwrites V
    }
}

template <int LFIX>
__global__ __launch_bounds__(D256_NT) void attn_bwd_d256_kernel(
    const uint16_t* __restrict__ qkvh, const float* __restrict__ logit_scale, const uint16_t* __restrict__ oh,
    const uint16_t* __restrict__ doh, const float* __restrict__ lse, const float* __restrict__ rnorm,
    uint16_t* __restrict__ dqkvh, float* __restrict__ dlogit, int Bw, int h, int L, int nW, int nww, int nwh, int mask_thr) {
    constexpr int LT = D256_LT, Lp = D256_LP, DP = D256_DP, SLAB = Lp * DP, NT = D256_NT;
    constexpr int CW = 64, NCH = DP / CW;                    // channel chunk: width and count
    constexpr int CT = CW / 16, CK = CW / 32;                // 16-column tiles / K = 32 steps per chunk
    constexpr int QP = CW + 8;                               // row pitch (elements) of the staged chunks: 144 bytes
    constexpr int DSP = Lp + 4;                              // row pitch of the [key][q] dS image
    constexpr int OFF_Q = 0, OFF_DO = OFF_Q + Lp * QP * 2, OFF_LSE = OFF_DO + Lp * QP * 2, OFF_DL = OFF_LSE + Lp * 4,
                  OFF_DS = OFF_DL + Lp * 4, OFF_RED = OFF_DS + Lp * DSP * 2, LDS_BYTES = OFF_RED + ((LT * 4 + 15) / 16) * 16;
    static_assert(OFF_DO % 16 == 0 && OFF_DS % 16 == 0 && LDS_BYTES <= 160 * 1024, "LDS layout");
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    uint16_t* const Qs = (uint16_t*)(lds + OFF_Q);           // phase 1: q^ chunk; phase 2: k^ chunk
    uint16_t* const dOs = (uint16_t*)(lds + OFF_DO);
    float* const LSEs = (float*)(lds + OFF_LSE);
    float* const DLs = (float*)(lds + OFF_DL);
    uint16_t* const dSb = (uint16_t*)(lds + OFF_DS);
    float* const red = (float*)(lds + OFF_RED);

    const int hd = blockIdx.y;
    const float tau = logit_scale[hd];
    const float sigma = clamped_logit_scale(tau);
    const float sc2 = sigma * SWV2_LOG2E;
    const int Lc = LFIX > 0 ? LFIX : L;
    float dsig = 0.f;
    // staging map of a chunk: 8 threads per row (one 16-byte piece each), 88 rows per pass, 2 passes
    constexpr int TPR = CW / 8, RPP = NT / TPR, PASSES = Lp / RPP;
    static_assert(Lp % RPP == 0, "staging map");

    for (int bw = blockIdx.x; bw < Bw; bw += gridDim.x) {
        // the lane-derived offsets are recomputed per window: hoisted out of the loop, the ~50 addresses of the unrolled tile loops
        // stay live across all phases and spill (the empty asm hides the thread index from loop-invariant code motion)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, tw = tid >> 6;             // wave tw owns key tile tw (phase 1) / query tile tw (phase 2)
        const int fr = lane & 15, g = lane >> 4;
        const int srow = tid / TPR, scc = tid % TPR;
        // one chunk of rows of slab `src` (element offset of the slab + chunk column) into LDS tile dst
        auto stage = [&](uint16_t* dst, size_t src) {
            bf16x8 r[PASSES];
#pragma unroll
            for (int p = 0; p < PASSES; ++p) r[p] = *(const bf16x8*)(qkvh + src + (size_t)(srow + RPP * p) * DP + scc * 8);
#pragma unroll
            for (int p = 0; p < PASSES; ++p) *(bf16x8*)(dst + (srow + RPP * p) * QP + scc * 8) = r[p];
        };
        const size_t slab0 = ((size_t)bw * h + hd) * 3 * SLAB, oslab = ((size_t)bw * h + hd) * SLAB;
        const int key = 16 * tw + fr;
        const bool do_mask = (mask_thr > 0) && last_window_row(bw, nW, nww, nwh);
        const bool kid = key >= mask_thr, key_ok = key < Lc;

        // ================= phase 1a / 1b, once per half of the query tiles (registers: 2 x 6 accumulators instead of 2 x 11) =================
        // S = Q K^T and dP = dO V^T summed over the four chunks (delta = rowsum(dO O) likewise, first half only); then P, dS as bf16
        // MFMA operands in registers and dS in the [key][q] image; dotk = sum_q dS cos for the k normalisation
        bf16x4 pb[LT], dsb[LT];
        float dotk = 0.f;
        int staged = -1;                                      // chunk of Q / dO in LDS (uniform)
        auto stage_qdo = [&](int c, bool delta) {
            __syncthreads();                                  // every wave is done with the staged chunk
#pragma unroll
            for (int p = 0; p < PASSES; ++p) {
                const int row = srow + RPP * p;
                const size_t off = (size_t)row * DP + CW * c + scc * 8;
                const uint4 sq = *(const uint4*)(qkvh + slab0 + off), sd = *(const uint4*)(doh + oslab + off);
                *(uint4*)(Qs + row * QP + scc * 8) = sq;
                *(uint4*)(dOs + row * QP + scc * 8) = sd;
                if (delta) {
                    const uint4 so = *(const uint4*)(oh + oslab + off);
                    const uint32_t a[4] = {sd.x, sd.y, sd.z, sd.w}, b[4] = {so.x, so.y, so.z, so.w};
                    float dl = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        dl = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(b[e] << 16), dl);
                        dl = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(b[e] & 0xffff0000u), dl);
                    }
                    dl = group_allsum<TPR>(dl);
                    if (scc == 0) DLs[row] = (c == 0 ? 0.f : DLs[row]) + dl;      // same thread, same row in every chunk
                }
            }
            if (delta && c == 0 && tid < Lp) LSEs[tid] = (tid < L) ? lse[((size_t)bw * h + hd) * Lp + tid] : 1.0e30f;   // padded queries: P = 0
            staged = c;
            __syncthreads();
        };
        auto half = [&](auto q0_c, auto nq_c, auto first_c) {
            constexpr int Q0 = decltype(q0_c)::value, NQ = decltype(nq_c)::value;
            constexpr bool FIRST = decltype(first_c)::value;
            f32x4 s[NQ], dp[NQ];
#pragma unroll
            for (int i = 0; i < NQ; ++i) { s[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
            for (int j = 0; j < NCH; ++j) {
                const int c = FIRST ? j : NCH - 1 - j;        // the second half starts on the chunk the first one left staged
                bf16x8 kf[CK], vf[CK];
#pragma unroll
                for (int kk = 0; kk < CK; ++kk) {
                    kf[kk] = *(const bf16x8*)(qkvh + slab0 + SLAB + (size_t)key * DP + CW * c + 32 * kk + 8 * g);
                    vf[kk] = *(const bf16x8*)(qkvh + slab0 + 2 * SLAB + (size_t)key * DP + CW * c + 32 * kk + 8 * g);
                }
                if (c != staged) stage_qdo(c, FIRST);
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    const int qt = Q0 + i;
#pragma unroll
                    for (int kk = 0; kk < CK; ++kk) {
                        const bf16x8 qa = *(const bf16x8*)(Qs + (16 * qt + fr) * QP + 32 * kk + 8 * g);
                        const bf16x8 da = *(const bf16x8*)(dOs + (16 * qt + fr) * QP + 32 * kk + 8 * g);
                        s[i] = mfma32(qa, kf[kk], s[i]);      // rows q = 16 qt + 4 g + r, column = key fr
                        dp[i] = mfma32(da, vf[kk], dp[i]);
                    }
                    __builtin_amdgcn_sched_barrier(0);        // no hoisting of every tile's fragments (registers)
                }
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int qt = Q0 + i;
                const f32x4 l4 = *(const f32x4*)(LSEs + 16 * qt + 4 * g);
                const f32x4 d4 = *(const f32x4*)(DLs + 16 * qt + 4 * g);
                f32x4 p, ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * qt + 4 * g + r;
                    float x = fmaf(s[i][r], sc2, -l4[r]);
                    x = key_ok ? x : SWV2_NEG_BIG;
                    if (do_mask) x += ((q >= mask_thr) != kid) ? (-100.f * SWV2_LOG2E) : 0.f;
                    const float pr = __builtin_amdgcn_exp2f(x);
                    p[r] = pr;
                    ds[r] = pr * (dp[i][r] - d4[r]);          // dS; d(cos) = sigma * dS is applied in the epilogues
                    dotk = fmaf(ds[r], s[i][r], dotk);
                }
                pb[qt] = f2bf4(p);
                dsb[qt] = f2bf4(ds);
                *(bf16x4*)(dSb + key * DSP + 16 * qt + 4 * g) = dsb[qt];
            }
        };
        half(std::integral_constant<int, 0>{}, std::integral_constant<int, (LT + 1) / 2>{}, std::true_type{});
        half(std::integral_constant<int, (LT + 1) / 2>{}, std::integral_constant<int, LT / 2>{}, std::false_type{});
        dotk = xor32_allsum(xor16_allsum(dotk));
        if (g == 0) dsig += dotk;                             // d logit_scale = sigma sum_{q,k} dS cos (see attn_bwd_kernel)

        // ================= phase 1c: dV^T += dO^T P, dK^T += Q^T dS per chunk, written at once =================
        {
            int tid = threadIdx.x;                            // (offsets recomputed for this phase, as above)
            asm volatile("" : "+v"(tid));
            const int lane = tid & 63, fr = lane & 15, g = lane >> 4, key = 16 * (tid >> 6) + fr;
            const float rks = rnorm[(((size_t)bw * h + hd) * 2 + 1) * Lp + key] * sigma;
#pragma unroll 1
            for (int c = 0; c < NCH; ++c) {                   // chunk 0 is still staged from the second half
                if (c != staged) stage_qdo(c, false);
                f32x4 dk[CT], dv[CT];
#pragma unroll
                for (int dt = 0; dt < CT; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int qt = 0; qt < LT; ++qt) {
#pragma unroll
                    for (int dt = 0; dt < CT; ++dt) {
                        const bf16x4 td = lds_tr_read(dOs + (16 * qt + 4 * g + (fr >> 2)) * QP + 16 * dt + (fr & 3) * 4);
                        const bf16x4 tq = lds_tr_read(Qs + (16 * qt + 4 * g + (fr >> 2)) * QP + 16 * dt + (fr & 3) * 4);
                        dv[dt] = mfma16(td, pb[qt], dv[dt]);
                        dk[dt] = mfma16(tq, dsb[qt], dk[dt]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int dt = 0; dt < CT; ++dt) {
                    const size_t off = (size_t)key * DP + CW * c + 16 * dt + 4 * g;
                    const bf16x4 kn = *(const bf16x4*)(qkvh + slab0 + SLAB + off);
                    *(bf16x4*)(dqkvh + slab0 + SLAB + off) = l2norm_bwd_out(dk[dt], kn, rks, dotk);
                    *(bf16x4*)(dqkvh + slab0 + 2 * SLAB + off) = f2bf4(dv[dt]);
                }
            }
        }

        // ================= phase 2: wave = query tile, dQ^T = sum_t K_t^T dS_t^T over the four K chunks =================
        {
            int tid = threadIdx.x;                            // (offsets recomputed for this phase, as above)
            asm volatile("" : "+v"(tid));
            const int lane = tid & 63, tw = tid >> 6, fr = lane & 15, g = lane >> 4, srow = tid / TPR, scc = tid % TPR;
            auto stage = [&](uint16_t* dst, size_t src) {
                bf16x8 r[PASSES];
#pragma unroll
                for (int p = 0; p < PASSES; ++p) r[p] = *(const bf16x8*)(qkvh + src + (size_t)(srow + RPP * p) * DP + scc * 8);
#pragma unroll
                for (int p = 0; p < PASSES; ++p) *(bf16x8*)(dst + (srow + RPP * p) * QP + scc * 8) = r[p];
            };
            constexpr int DT = DP / 16;
            f32x4 dq[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            auto frag = [&](int t, bf16x4 (&kt_)[CT], bf16x4& ds_) {
                const int row = 16 * t + 4 * g + (fr >> 2);
#pragma unroll
                for (int dt = 0; dt < CT; ++dt) kt_[dt] = lds_tr_read(Qs + row * QP + 16 * dt + (fr & 3) * 4);     // rows d, col key
                ds_ = lds_tr_read(dSb + row * DSP + 16 * tw + (fr & 3) * 4);                                    // B[k = key][n = q]
            };
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                __syncthreads();                              // phase 1 (or the previous chunk) is done with the Q tile
                stage(Qs, slab0 + SLAB + CW * c);
                __syncthreads();
#pragma unroll 1
                for (int t = 0; t + 1 < LT; t += 2) {
                    bf16x4 k0[CT], k1[CT], d0, d1;
                    frag(t, k0, d0);
                    frag(t + 1, k1, d1);
#pragma unroll
                    for (int dt = 0; dt < CT; ++dt)
                        dq[CT * c + dt] = mfma32(__builtin_shufflevector(k0[dt], k1[dt], 0, 1, 2, 3, 4, 5, 6, 7),
                                                 __builtin_shufflevector(d0, d1, 0, 1, 2, 3, 4, 5, 6, 7), dq[CT * c + dt]);
                }
                if (LT & 1) {
                    bf16x4 k0[CT], d0;
                    frag(LT - 1, k0, d0);
#pragma unroll
                    for (int dt = 0; dt < CT; ++dt) {
                        const f32x4 tail = mfma16(k0[dt], d0, (f32x4){0.f, 0.f, 0.f, 0.f});      // own accumulator (attn_bwd_kernel)
                        dq[CT * c + dt] += tail;
                    }
                }
            }
            const int q = 16 * tw + fr;
            const float rq = rnorm[(((size_t)bw * h + hd) * 2 + 0) * Lp + q] * sigma;
            float dot = 0.f;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x4 qn = *(const bf16x4*)(qkvh + slab0 + (size_t)q * DP + 16 * dt + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) dot = fmaf(dq[dt][r], bf2f(qn[r]), dot);
            }
            dot = xor32_allsum(xor16_allsum(dot));
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x4 qn = *(const bf16x4*)(qkvh + slab0 + (size_t)q * DP + 16 * dt + 4 * g);
                *(bf16x4*)(dqkvh + slab0 + (size_t)q * DP + 16 * dt + 4 * g) = l2norm_bwd_out(dq[dt], qn, rq, dot);
            }
        }
        __syncthreads();                                      // the next window's staging overwrites the tiles and the dS image
    }

    // ---- one atomic per workgroup for the logit scale
    const int tid = threadIdx.x, lane = tid & 63, tw = tid >> 6;
    dsig = wave_sum(dsig);
    if (lane == 0) red[tw] = dsig;
    __syncthreads();
    if (tid == 0 && tau <= SWV2_LN100) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < LT; ++i) t += red[i];
        atomicAdd(dlogit + hd, t * sigma);
    }
}

// 0 = launch, negative = error
int d256_check(const swv2_attn_args* a, int Lp) {
    if (a->bias) {
        swv2_set_error("attention: no CPB bias at head_dim=%d (the 256-column kernels have no table)", a->head_dim);
        return SWV2_ERR_UNSUPPORTED;
    }
    SWV2_CHECK_ARG(Lp == D256_LP, "attention: head_dim=%d needs the %d-row window layout (got Lp=%d)", a->head_dim, D256_LP, Lp);
    return 0;
}

dim3 d256_grid(const swv2_attn_args* a) {
    // one workgroup (11 waves) per CU: persistent over the windows of its head
    int chunks = 256 / a->heads;
    if (chunks < 1) chunks = 1;
    if (chunks > a->Bw) chunks = a->Bw;
    return dim3(chunks, a->heads);
}

}  // namespace

// the kernel pair for 256-channel heads, called by swv2_attn_fwd / swv2_attn_bwd (attn.hip) at DP = 256: 0 = launched, negative = error
int swv2_attn_fwd_d256(const swv2_attn_args* a, int Lp, void* stream) {
    const int rc = d256_check(a, Lp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nW = a->nwh * a->nww;
#define SWV2_LAUNCH_D256(LFIX)                                                                                                        \
    hipLaunchKernelGGL((attn_fwd_d256_kernel<LFIX>), d256_grid(a), dim3(D256_NT), 0, st, (const uint16_t*)a->qkvh, a->logit_scale, \
                       (uint16_t*)a->oh, a->lse, a->Bw, a->heads, a->L, nW, a->nww, a->nwh, a->mask_thr)
    if (attn_lfix_other(a->L) == 162) SWV2_LAUNCH_D256(162); else SWV2_LAUNCH_D256(0);
#undef SWV2_LAUNCH_D256
    SWV2_CHECK_LAUNCH("swv2_attn_fwd");
    return SWV2_OK;
}

int swv2_attn_bwd_d256(const swv2_attn_args* a, int Lp, void* stream) {
    const int rc = d256_check(a, Lp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nW = a->nwh * a->nww;
#define SWV2_LAUNCH_D256(LFIX)                                                                                                         \
    hipLaunchKernelGGL((attn_bwd_d256_kernel<LFIX>), d256_grid(a), dim3(D256_NT), 0, st, (const uint16_t*)a->qkvh, a->logit_scale,  \
                       (const uint16_t*)a->oh, (const uint16_t*)a->doh, a->lse, a->rnorm, (uint16_t*)a->dqkvh, a->dlogit_scale, a->Bw, \
                       a->heads, a->L, nW, a->nww, a->nwh, a->mask_thr)
    if (attn_lfix_other(a->L) == 162) SWV2_LAUNCH_D256(162); else SWV2_LAUNCH_D256(0);
#undef SWV2_LAUNCH_D256
    SWV2_CHECK_LAUNCH("swv2_attn_bwd");
    return SWV2_OK;
}
