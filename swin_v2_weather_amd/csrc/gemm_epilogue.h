// Epilogues of the GEMM engine's NT products: the epilogue descriptor and its kinds (EpiDesc, E_*, Epi<>, make_epi), the staging
// pitch EP, the head-major epilogues (heads_item*) and the epilogue of the 256 x 256 kernels (wide_epilogue).
// Included by gemm.hip, gemm_wide.hip, gemm_rw.hip (the resident qkv kernel) and gemm_tn.hip (the wide weight-gradient kernel's partial tiles).
#pragma once
#include <type_traits>
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Epilogues: tile(stage, m0, n0, lane) consumes a 16-row x 64-col fp32 sub-tile held in wave-private LDS
// (pitch EP floats): rows m0..m0+15, cols n0..n0+63 of C.
// ------------------------------------------------------------------------------------------------
constexpr int EP = 68;     // staging pitch in floats

struct EpiDesc {
    void* out;              // primary output
    const float* bias;      // [N] or null
    const void* aux;        // kind specific (pre-activation for GELU', skip input, ...)
    float* aux_out;         // kind specific second output (rnorm)
    const int32_t* rowidx;  // optional scatter table: logical row -> destination row, <0 = skip
    long ld;                // output row pitch (elements)
    int M, N;
    int p0, p1, p2, p3, p4;
    uint32_t mg0, mg1, mg2; // fdiv magics (make_epi)
    // E_UNPATCH_LOSS
    const float* loss_tar; const float* loss_qw; float* loss_part; uint16_t* loss_resid; int q0, q1, q2, q3;
};

enum { E_BF16 = 0, E_F32 = 1, E_QKV_HEADS = 2, E_GELU_GRAD = 3, E_UNPATCH = 4, E_HEADS = 5, E_F32_ACC = 6, E_BF16_GELU = 7,
       E_UNPATCH_LOSS = 8, E_UNPATCH_LOSS_SKIP = 9 };      // (9: the same epilogue with a skip tensor; compile-time, see the kernel)

template <int KIND> struct Epi;

// The row-major epilogues share one lane map: lane -> (row r = lane / 4, 16 columns from c0) of the sub-tile = element (m, n) of C,
// written to row dst (SCATTER: through d.rowidx where the product has one).  false: outside the matrix, or a skipped row
struct RowLane { int r, c0, m, n; long dst; };
template <bool SCATTER>
__device__ __forceinline__ bool row_lane(const EpiDesc& d, int m0, int n0, int lane, RowLane& q) {
    q.r = lane >> 2; q.c0 = (lane & 3) * 16; q.m = m0 + q.r; q.n = n0 + q.c0;
    if (q.m >= d.M || q.n >= d.N) return false;
    q.dst = q.m;
    if constexpr (SCATTER) {
        if (d.rowidx) { q.dst = d.rowidx[q.m]; if (q.dst < 0) return false; }
    }
    return true;
}
// the lane's 16 staged values
__device__ __forceinline__ void staged16(const float* st, const RowLane& q, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4*)(v + 4 * i) = *(const f32x4*)(st + q.r * EP + q.c0 + 4 * i);
}
// row-major bf16 store (+bias)
template <> struct Epi<E_BF16> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        RowLane q;
        if (!row_lane<true>(d, m0, n0, lane, q)) return;
        const int n = q.n;
        float v[16];
        staged16(st, q, v);
        if (d.bias) {
            if (n + 16 <= d.N) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 b4 = *(const f32x4*)(d.bias + n + 4 * i);
                    v[4 * i] += b4[0]; v[4 * i + 1] += b4[1]; v[4 * i + 2] += b4[2]; v[4 * i + 3] += b4[3];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] += (n + i < d.N) ? d.bias[n + i] : 0.f;
            }
        }
        uint16_t* o = (uint16_t*)d.out + q.dst * d.ld + n;
        if (n + 16 <= d.N) {
            *(uint4*)o = pack8(v);
            *(uint4*)(o + 8) = pack8(v + 8);
        } else {
            for (int i = 0; i < 16 && n + i < d.N; ++i) o[i] = f2bf(v[i]);
        }
    }
};
// fc1 of the Mlp: out = acc + bias (bf16 pre-activation), aux_out = GELU(out) (bf16), same row-major layout
template <> struct Epi<E_BF16_GELU> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        RowLane q;
        if (!row_lane<false>(d, m0, n0, lane, q)) return;
        const int n = q.n;
        float v[16], gl[16];
        staged16(st, q, v);
        if (d.bias) {
            if (n + 16 <= d.N) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 b4 = *(const f32x4*)(d.bias + n + 4 * i);
                    v[4 * i] += b4[0]; v[4 * i + 1] += b4[1]; v[4 * i + 2] += b4[2]; v[4 * i + 3] += b4[3];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] += (n + i < d.N) ? d.bias[n + i] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) gl[i] = gelu_f(bf2f(f2bf(v[i])));   // GELU of the stored (bf16) pre-activation
        uint16_t* o = (uint16_t*)d.out + q.dst * d.ld + n;
        uint16_t* o2 = (uint16_t*)d.aux_out + q.dst * d.ld + n;
        if (n + 16 <= d.N) {
            *(uint4*)o = pack8(v);
            *(uint4*)(o + 8) = pack8(v + 8);
            *(uint4*)o2 = pack8(gl);
            *(uint4*)(o2 + 8) = pack8(gl + 8);
        } else {
            for (int i = 0; i < 16 && n + i < d.N; ++i) { o[i] = f2bf(v[i]); o2[i] = f2bf(gl[i]); }
        }
    }
};
// row-major fp32 store (+bias) (+aux: an fp32 tensor of the output's shape added at the destination row, e.g. the
// gradient that arrives over the residual connection)
template <> struct Epi<E_F32> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        RowLane q;
        if (!row_lane<true>(d, m0, n0, lane, q)) return;
        const int n = q.n;
        float* o = (float*)d.out + q.dst * d.ld + n;
        const float* ax = d.aux ? (const float*)d.aux + q.dst * d.ld + n : nullptr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 v = *(const f32x4*)(st + q.r * EP + q.c0 + 4 * i);
            if (n + 4 * i + 4 <= d.N) {
                if (d.bias) v += *(const f32x4*)(d.bias + n + 4 * i);
                if (ax) v += *(const f32x4*)(ax + 4 * i);
                *(f32x4*)(o + 4 * i) = v;
            } else {
                for (int j = 0; j < 4 && n + 4 * i + j < d.N; ++j)
                    o[4 * i + j] = v[j] + (d.bias ? d.bias[n + 4 * i + j] : 0.f) + (ax ? ax[4 * i + j] : 0.f);
            }
        }
    }
};
// fp32 accumulate into the destination (dx of the second branch summed into the first), no bias
template <> struct Epi<E_F32_ACC> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        RowLane q;
        if (!row_lane<true>(d, m0, n0, lane, q)) return;
        float* o = (float*)d.out + q.dst * d.ld + q.n;
        for (int i = 0; i < 16 && q.n + i < d.N; ++i) o[i] += st[q.r * EP + q.c0 + i];
    }
};
// q/k/v split into the head-major window layout (HeadLayout, gemm_common.h) with L2-normalised q and k (swinv2_global.py:300-304).
// Logical column n, logical row m as there: padded columns are exact zeros (swv2_prep_weight), rows t >= L are padding and are
// written as zeros.  p0 = heads, p2 = Lp, p3 = DP, p4 = L, mg0 .. mg2 = the layout's magics (make_epi) ; out = qkvh ; aux_out = rnorm ;
// bias is padded like n.  S = 3 parts with normalisation of parts 0 and 1 (E_QKV_HEADS) or 1 without (E_HEADS).
// heads_item and heads_item_wide keep their own text of the layout (see HeadLayout).  The layout as an epilogue sees it (the resident
// qkv kernel of gemm_rw.hip): S and DP are the caller's, compile-time values fold away
__device__ __forceinline__ HeadLayout epi_layout(const EpiDesc& d, int S, int DP) { return {d.p0, S, d.p2, DP, d.mg0, d.mg1, d.mg2}; }

template <int DPc, bool NORM>
__device__ __forceinline__ void heads_item(const EpiDesc& d, const float* st, int m0, int n0, int lane) {
    const int h = d.p0, Lp = d.p2, L = d.p4, S = NORM ? 3 : 1;
    constexpr int SLOTS = 64 / DPc;                   // heads per 64-column sub-tile
    for (int it = lane; it < 16 * SLOTS; it += 64) {
        const int r = it & 15, slot = it >> 4;
        const int nb = n0 + slot * DPc, m = m0 + r;
        if (m >= d.M || nb >= d.N) continue;
        const int ph = nb / DPc, part = (h == 1) ? ph : fdiv(ph, h, d.mg1), hd = ph - part * h;
        const int bw = fdiv(m, Lp, d.mg0), t = m - bw * Lp;
        const bool valid = t < L;
        float v[DPc];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < DPc; j += 4) {
            f32x4 x = *(const f32x4*)(st + r * EP + slot * DPc + j);
            if (d.bias) x += *(const f32x4*)(d.bias + nb + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[j + e] = valid ? x[e] : 0.f;
                ss = fmaf(v[j + e], v[j + e], ss);
            }
        }
        float rn = 1.f;
        if (NORM && part < 2) {
            rn = 1.f / fmaxf(sqrtf(ss), 1e-12f);
            d.aux_out[(((long)bw * h + hd) * 2 + part) * Lp + t] = valid ? rn : 0.f;
        }
        uint16_t* o = (uint16_t*)d.out + ((((long)bw * h + hd) * S + part) * Lp + t) * DPc;
#pragma unroll
        for (int j = 0; j < DPc; j += 8) {
            float w[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = v[j + e] * rn;
            *(uint4*)(o + j) = pack8(w);
        }
    }
}
// DP = 96 / 128 / 256 (head dims 65 .. 128, 256): a wave's 64-column sub-tile is PART of a head, so the squared norm cannot be finished
// here.  Each 64-column piece adds its partial sum of squares into rnorm (zeroed by the caller) by a float atomic: two
// addends per row at DP = 128 (order-independent, so bit-reproducible), up to six at 96 and four at 256 (the order, and so the
// last bit of the sum and of q^ / k^, varies from run to run).  It writes the UN-normalised bf16 values; swv2_qk_normalize then turns the sums into 1 / |.| and rescales q, k in
// place (one extra bf16 rounding of q^, k^ compared with the narrow-head epilogue).  lane = (row, 16-column quarter).
// PB: the lane's 16 bias values were loaded by the caller (once per tile: the wide kernels; a load inside this function sits
// under a condition and makes the compiler wait for every earlier store with s_waitcnt vmcnt(0)); zeros without a bias
template <bool NORM, bool PB = false>
__device__ __forceinline__ void heads_item_wide(const EpiDesc& d, const float* st, int m0, int n0, int lane, const f32x4* pb = nullptr) {
    const int h = d.p0, Lp = d.p2, L = d.p4, S = NORM ? 3 : 1;
    const int r = lane & 15, qd = lane >> 4, nb = n0 + 16 * qd, m = m0 + r;
    const bool in = (m < d.M) && (nb < d.N);
    const int DPv = d.p3, ph = DPv == 128 ? (nb >> 7) : fdiv(nb, DPv, d.mg2), part = (h == 1) ? ph : fdiv(ph, h, d.mg1), hd = ph - part * h;
    const int bw = fdiv(min(m, d.M - 1), Lp, d.mg0), t = min(m, d.M - 1) - bw * Lp;
    const bool valid = in && t < L;
    float v[16];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
        f32x4 x = *(const f32x4*)(st + r * EP + 16 * qd + j);
        if constexpr (PB) x += pb[j >> 2];
        else if (d.bias && in) x += *(const f32x4*)(d.bias + nb + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[j + e] = valid ? x[e] : 0.f;
            ss = fmaf(v[j + e], v[j + e], ss);
        }
    }
    if (NORM) {
        if (DPv >= 128) {                 // the wave's 64 columns lie in ONE head: one addend per row (four per row at DP = 256:
                                          // their order, and so the last bit of the sum, is not fixed)
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            if (in && qd == 0 && part < 2 && valid) atomicAdd(d.aux_out + (((long)bw * h + hd) * 2 + part) * Lp + t, ss);
        } else {                          // 96-wide heads: a 64-column sub-tile may straddle two heads -- one addend per 16-column group
            if (in && part < 2 && valid) atomicAdd(d.aux_out + (((long)bw * h + hd) * 2 + part) * Lp + t, ss);
        }
    }
    if (in) {
        uint16_t* o = (uint16_t*)d.out + ((((long)bw * h + hd) * S + part) * Lp + t) * DPv + (nb - ph * DPv);
        *(uint4*)o = pack8(v);
        *(uint4*)(o + 8) = pack8(v + 8);
    }
}
template <> struct Epi<E_QKV_HEADS> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        if (d.p3 == 16) heads_item<16, true>(d, st, m0, n0, lane);
        else if (d.p3 == 32) heads_item<32, true>(d, st, m0, n0, lane);
        else if (d.p3 == 64) heads_item<64, true>(d, st, m0, n0, lane);
        else heads_item_wide<true>(d, st, m0, n0, lane);
    }
};
// heads split without normalisation: [Bw][h][1][Lp][DP] (gradient of the merged attention output)
template <> struct Epi<E_HEADS> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        if (d.p3 == 16) heads_item<16, false>(d, st, m0, n0, lane);
        else if (d.p3 == 32) heads_item<32, false>(d, st, m0, n0, lane);
        else if (d.p3 == 64) heads_item<64, false>(d, st, m0, n0, lane);
        else heads_item_wide<false>(d, st, m0, n0, lane);
    }
};
// dh = (acc) * GELU'(pre-activation) ; aux = pre-activation bf16 [M][N] row-major, same pitch as out
template <> struct Epi<E_GELU_GRAD> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        RowLane q;
        if (!row_lane<false>(d, m0, n0, lane, q)) return;
        const int n = q.n;
        const uint16_t* pre = (const uint16_t*)d.aux + q.dst * d.ld + n;
        uint16_t* o = (uint16_t*)d.out + q.dst * d.ld + n;
        float v[16], hv[16];
        staged16(st, q, v);
        if (n + 16 <= d.N) {
            unpack8(*(const uint4*)pre, hv);
            unpack8(*(const uint4*)(pre + 8), hv + 8);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] *= gelu_grad_f(hv[i]);
            *(uint4*)o = pack8(v);
            *(uint4*)(o + 8) = pack8(v + 8);
        } else {
            for (int i = 0; i < 16 && n + i < d.N; ++i) o[i] = f2bf(v[i] * gelu_grad_f(bf2f(pre[i])));
        }
    }
};
// head Linear + un-patchify (+ residual skip), swinv2_global.py:784-802.  The bf16 head weight is stored with its
// rows permuted to n' = c*16 + p*4 + q (swv2_cast_weights), so 16 consecutive columns are one channel's 4x4 patch:
//   y[b][c][4i+p][4j+q] = acc[m=(b,i,j)][c*16 + p*4 + q] (+ skip[b][c][4i+p][4j+q])
// p0 = Cout, p1 = H, p2 = W, p3 = Cskip (channels of the skip tensor, 0 = no skip) ; aux = skip ; out = y
// p4 = channels per sample of the tensor `out` points into (0 = Cout); aux_out = optional SECOND destination with ld
// channels per sample -- the autoregressive rollout writes a step's prediction straight into the concatenated result and
// into the next step's input buffer (helpers.py:26-41: two torch.cat copies of ~300 MB per sample and step otherwise)
template <> struct Epi<E_UNPATCH> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float* st, int m0, int n0, int lane) const {
        const int Cout = d.p0, H = d.p1, W = d.p2, Cs = d.p3, gw = W >> 2, gh = H >> 2;
        const int Ct = d.p4 ? d.p4 : Cout;
        // 16 rows x 4 channels x 4 p = 256 float4 items; lane -> row fastest so stores run along W
        for (int it = lane; it < 256; it += 64) {
            const int r = it & 15, cp = it >> 4, cl = cp >> 2, p = cp & 3;
            const int m = m0 + r, c = (n0 >> 4) + cl;
            if (m >= d.M || c >= Cout) continue;
            const int b = fdiv(m, gh * gw, d.mg0), ij = m - b * gh * gw, i = fdiv(ij, gw, d.mg1), j = ij - i * gw;
            f32x4 v = *(const f32x4*)(st + r * EP + cl * 16 + p * 4);
            if (Cs) v += *(const f32x4*)((const float*)d.aux + (((long)b * Cs + c) * H + 4 * i + p) * W + 4 * j);
            *(f32x4*)((float*)d.out + (((long)b * Ct + c) * H + 4 * i + p) * W + 4 * j) = v;
            if (d.aux_out) *(f32x4*)((float*)d.aux_out + (((long)b * d.ld + c) * H + 4 * i + p) * W + 4 * j) = v;
        }
    }
};

// un-patchify (+ skip) that also evaluates the geometric l2 loss of the prediction while it is in registers
// (losses.py:188-206: sum_hw q[h] (prd - tar)^2 and sum_hw q[h] tar^2 per (sample, channel); grids.py:115-117) and leaves the
// quadrature-weighted residual q[h] (prd - tar) as a bf16 [M][SWV2_LOSS_RESID_PITCH(N)] matrix in the GEMM's own layout for the head's backward.
// The reference (and rounds 1 - 2 here) read the 303 MB / sample prediction back twice (loss, loss gradient) and wrote a
// gradient of the same size that both backward GEMMs of the head re-read through the 4 x 4 patch gather.
//   row_of      : what a lane has to know about its row of a 16-row tile (sample, image position, quadrature weight), once per kernel
//   load_tar    : the lane's four target float4 of one 16 x 64 tile (four channels), requested a whole N tile ahead
//   tile_loss_t : one 16 x 64 tile on the accumulators of the TRANSPOSED product: lane = (token fr, image row p = g), register r = q, one
//                 channel per 16 x 16 tile; ls[2k], ls[2k + 1] = channel k's partial sums; only the bf16 residual is staged through LDS
//   flush       : per (N tile, 32-row group) wave-reduce the sums (lane swaps + DPP) and STORE them as the group's partial sums
//                 (swv2_loss_part_reduce adds the groups of a sample in a fixed order: the loss value is bit-reproducible).  The
//                 first version added them to the (sample, channel) sums with atomics: 146 addresses hit by 80 K wave-level
//                 atomics made the kernel 1071 us instead of 138 us.
// Rollouts (round 5): `out` may be a channel block of a larger tensor (p4 channels per sample, dump offset q2) and aux_out a second
// destination (the next step's input) written from the same registers.
template <> struct Epi<E_UNPATCH_LOSS> {
    EpiDesc d;
    __device__ __forceinline__ void tile(const float*, int, int, int) const {}
    // What one 16 x 64 tile needs from global memory: this lane's four target float4 (its row / image row, the four channels
    // of the wave's column block) and its quadrature weight.  Requested ONE TILE AHEAD of its use -- before the previous tile's
    // stores are issued, across the MFMA phase between two N tiles -- because vmcnt retires in order and counts stores: waiting
    // for a load that was issued behind a store is waiting for that store to complete (SQ_WAIT_ANY was 79 % of the kernel's
    // wave-cycles with the loads at the top of each tile, profiles/r03_pmc_wait.json).  Everything in load_tar / tile_loss is
    // straight-line code, so the waits are counted vmcnt(N): masked rows / channels load from clamped addresses and store into
    // small dump areas BEHIND the prediction and the residual (same scalar base + 32-bit offset; a select between two base
    // pointers needs 64-bit per-lane addresses, and the kernel spills).
    struct Tar { f32x4 t[4]; float q; };
    // what a lane needs to know about its row of a 16-row tile (token -> sample, image position): the same for every N tile, so the
    // kernel resolves it ONCE per row tile in front of its main loop (inside the epilogue it was ~50 integer instructions per tile)
    struct Row { uint32_t pix, tbase, ybase, nbase, sbase; float q; int b; bool ok; };
    __device__ __forceinline__ Row row_of(int m0, int lane) const {
        const int H = d.p1, W = d.p2, gw = W >> 2, gh = H >> 2;
        const int r = lane & 15, p = lane >> 4, m = m0 + r, mc = min(m, d.M - 1);
        const int b = fdiv(mc, gh * gw, d.mg0), ij = mc - b * gh * gw, i = fdiv(ij, gw, d.mg1), j = ij - i * gw;
        Row o;
        o.pix = (uint32_t)((4 * i + p) * W + 4 * j);
        o.tbase = (uint32_t)b * d.q0 + d.q1;                    // first target channel of the sample
        o.ybase = (uint32_t)b * (d.p4 ? d.p4 : d.p0);           // p4: channels per sample of the tensor `out` points into (rollouts)
        o.nbase = (uint32_t)b * (uint32_t)d.ld;                 // second destination (aux_out), ld channels per sample
        o.sbase = (uint32_t)b * d.p3;
        o.q = d.loss_qw[4 * i + p];
        o.b = b;
        o.ok = m < d.M;
        return o;
    }
    __device__ __forceinline__ void load_tar(const Row& rw, int n0, Tar& o) const {
        const int Cout = d.p0;
        const uint32_t plane = (uint32_t)(d.p1 * d.p2);
        o.q = rw.q;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = (uint32_t)min((n0 >> 4) + k, Cout - 1);
            o.t[k] = *(const f32x4*)(d.loss_tar + ((rw.tbase + c) * plane + rw.pix));
        }
    }
    // The same step on the accumulators of the TRANSPOSED product (D^T = W X^T: lane (token fr, image row p = g) holds the four
    // values q = 0..3 of one channel per 16 x 16 tile -- exactly the float4 of y / tar / skip this lane touches), so the prediction
    // never passes through the LDS: round 5 measured the staged form at 190 us of epilogue work with every memory stream removed
    // (16 + 12 LDS instructions and ~200 vector instructions per 16 x 64 tile; 422 us with the streams).  Only the bf16 residual is
    // staged (one 8-byte write per channel, two 16-byte reads) so that its rows leave as 128 contiguous bytes.
    template <bool HAS_SKIP>
    __device__ __forceinline__ void tile_loss_t(const f32x4 (&acc)[4], uint16_t* st16, const Row& rw, int m0, int n0, int lane, float (&ls)[8],
                                                float (&ls2)[8], int b0, const Tar& in) const {
        constexpr int RP = 72;                                   // bf16 pitch of the residual staging tile [16][64]
        const int Cout = d.p0;
        const int r = lane & 15, p = lane >> 4;
        const uint32_t plane = (uint32_t)(d.p1 * d.p2);
        const float q = in.q;
        float* outp = (float*)d.out;
        // residual rows have a pitch of whole 128-byte lines (SWV2_LOSS_RESID_PITCH): with N = 1168 elements per row every 128-byte
        // piece straddled two lines and the head's two backward products fetched 644 / 708 MB for 368 / 335 MB (profiles/r05_pmc_hbm.json)
        const uint32_t RPITCH = (uint32_t)SWV2_LOSS_RESID_PITCH(d.N);
        const uint32_t ydump = (uint32_t)d.q2 + lane * 4, ndump = (uint32_t)d.q3 + lane * 4, rdump = (uint32_t)d.M * RPITCH + lane * 16;
        const bool same = (rw.b == b0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = (n0 >> 4) + k;
            const bool ok = rw.ok && c < Cout;
            f32x4 v = acc[k];
            if constexpr (HAS_SKIP) v += *(const f32x4*)((const float*)d.aux + ((rw.sbase + min(c, Cout - 1)) * plane + rw.pix));
            *(f32x4*)(outp + (ok ? (rw.ybase + c) * plane + rw.pix : ydump)) = v;
            // rollouts: the next step's input buffer gets the prediction from the same registers (wave-uniform branch around stores
            // only: the counted waits of the common path are unaffected)
            if (d.aux_out) *(f32x4*)(d.aux_out + (ok ? (rw.nbase + c) * plane + rw.pix : ndump)) = v;
            const f32x4 dd = v - in.t[k];
            const float e0 = q * (dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] + dd[3] * dd[3]);
            const float e1 = q * (in.t[k][0] * in.t[k][0] + in.t[k][1] * in.t[k][1] + in.t[k][2] * in.t[k][2] + in.t[k][3] * in.t[k][3]);
            // rows of the group's first sample -> ls, rows of the next sample (groups that straddle a sample boundary) -> ls2
            ls[2 * k] += (ok && same) ? e0 : 0.f;
            ls[2 * k + 1] += (ok && same) ? e1 : 0.f;
            ls2[2 * k] += (ok && !same) ? e0 : 0.f;
            ls2[2 * k + 1] += (ok && !same) ? e1 : 0.f;
            *(bf16x4*)(st16 + r * RP + 16 * k + 4 * p) = f2bf4(q * dd);
        }
        // residual rows out as bf16, row-major: lane -> (row lane / 4, 16 columns), 128 contiguous bytes per row
        const int r2 = lane >> 2, c0 = (lane & 3) * 16, m2 = m0 + r2, n = n0 + c0;
        const uint4 w0 = *(const uint4*)(st16 + r2 * RP + c0), w1 = *(const uint4*)(st16 + r2 * RP + c0 + 8);
        uint16_t* o = d.loss_resid + ((m2 < d.M && n < d.N) ? (uint32_t)m2 * RPITCH + n : rdump);
        *(uint4*)o = w0;
        *(uint4*)(o + 8) = w1;
    }
    // loss_part[group][slot][Cout][2]: slot 0 = rows of the sample of the group's first row, slot 1 = rows of the following
    // sample (zero unless the group straddles a boundary).  Lane 63 holds the DPP sums and stores 8 floats per slot.
    // Sums of eight per-lane values over the wave with the gfx950 lane swaps: v_permlane32_swap folds the two halves of a value pair
    // into one register (lanes 0..31 = the first value, 32..63 = the second), v_permlane16_swap the 16-lane rows of two such registers,
    // four DPP steps finish the rows: 6 swaps + 6 + 8 adds for 8 values (six DPP steps per value were 96 moves + 96 adds per flush).
    // Row q = lane >> 4 of x0 then holds the sum of value (0, 2, 1, 3)[q], of x1 that of value 4 + (0, 2, 1, 3)[q], in every lane.
    static __device__ __forceinline__ void wave_sum8_rows(const float (&v)[8], float& x0, float& x1) {
        // inline assembly on purpose: with this toolchain (ROCm 7.2 clang) element 1 of __builtin_amdgcn_permlane{32,16}_swap's result
        // pair is compiled as element 0 again (`v_add_f32 v9, v10, v10` behind the swap -- found by the sums coming out 20 % low and
        // confirmed in a standalone kernel); the s_nop 1 in front is the wait the compiler itself puts between a vector write and the swap
        auto fold32 = [](float a, float b) {
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
            return a + b;
        };
        auto fold16 = [](float a, float b) {
            asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
            return a + b;
        };
        auto rowsum = [](float x) {
            auto dpp = [](float y, auto ctrl) {
                return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), decltype(ctrl)::value, 0xf, 0xf, true));
            };
            x += dpp(x, std::integral_constant<int, 0xb1>{});      // quad_perm [1,0,3,2]
            x += dpp(x, std::integral_constant<int, 0x4e>{});      // quad_perm [2,3,0,1]
            x += dpp(x, std::integral_constant<int, 0x141>{});     // row_half_mirror
            x += dpp(x, std::integral_constant<int, 0x140>{});     // row_mirror
            return x;
        };
        x0 = rowsum(fold16(fold32(v[0], v[1]), fold32(v[2], v[3])));
        x1 = rowsum(fold16(fold32(v[4], v[5]), fold32(v[6], v[7])));
    }
    // loss_part[group][slot][Cout][2]: slot 0 = rows of the sample of the group's first row, slot 1 = rows of the following
    // sample.  swv2_loss_part_reduce reads slot 1 only of the group in FRONT of a sample's first group, so slot 1 is written (zeros
    // unless the group straddles the boundary) only by groups whose successor row belongs to another sample (`edge`, wave-uniform: one
    // group in ~2 000).  The first lane of row q stores its two values; every other lane -- and channels past Cout / rows past M --
    // stores the same instruction into the dump area behind the residual, so the common path has no branch around memory operations.
    template <int GR> __device__ __forceinline__ void flush(float (&ls)[8], float (&ls2)[8], bool edge, int m_first, int n0, int lane) const {
        const int c0 = n0 >> 4, qr = lane >> 4, vi = ((qr & 1) << 1) | (qr >> 1);
        float* const dump = (float*)(d.loss_resid + (size_t)d.M * SWV2_LOSS_RESID_PITCH(d.N)) + 2 * lane;
        float* const sp = d.loss_part + ((long)(m_first / GR) * 2 * d.p0 + c0) * 2;
        const bool lead = (lane & 15) == 0 && m_first < d.M;
        const bool ok0 = lead && c0 + (vi >> 1) < d.p0, ok1 = lead && c0 + 2 + (vi >> 1) < d.p0;
        float x0, x1;
        wave_sum8_rows(ls, x0, x1);
        *(ok0 ? sp + vi : dump) = x0;
        *(ok1 ? sp + 4 + vi : dump + 1) = x1;
        if (edge) {
            wave_sum8_rows(ls2, x0, x1);
            *(ok0 ? sp + 2 * d.p0 + vi : dump) = x0;
            *(ok1 ? sp + 2 * d.p0 + 4 + vi : dump + 1) = x1;
        }
    }
};

template <> struct Epi<E_UNPATCH_LOSS_SKIP> : Epi<E_UNPATCH_LOSS> {};

// the (loader, epilogue) pairs the special kernels are instantiated for: gemm.hip's selector tests them at run time, the launchers at compile time
constexpr bool qkv_pair(int ak, int ek) { return ak == A_F32 && ek == E_QKV_HEADS; }      // a block's qkv product
constexpr bool dx_pair(int ak, int ek) { return ak == A_HEADS && ek == E_F32; }           // a block's d(qkv) -> dx product
constexpr bool loss_epi(int ek) { return ek == E_UNPATCH_LOSS || ek == E_UNPATCH_LOSS_SKIP; }
constexpr bool wide_pair(int ak, int ek) {
    return (ak == A_F32 || ak == A_BF16 || ak == A_HEADS) &&
           (ek == E_BF16 || ek == E_F32 || ek == E_F32_ACC || ek == E_QKV_HEADS || ek == E_HEADS || ek == E_GELU_GRAD || ek == E_BF16_GELU);
}
constexpr bool dma_loader(int ak) { return ak == A_BF16 || ak == A_HEADS; }               // raw bf16 in memory: LDS-DMA can fetch it

// Epilogue of a wave's 128 x 64 accumulator tile in the wide kernels.  Epi<>::tile loads its bias / residual / pre-activation
// operands under conditions, which costs an s_waitcnt vmcnt(0) per 16-row sub-tile -- a wait for the acknowledgement of every
// store of the previous sub-tile (measured: 20 us per tile for 256 KB, half the kernel at K = 768).  Here everything a lane needs
// for all eight sub-tiles is loaded up front (bias: the lane's columns are the same in every sub-tile; scatter rows), the
// per-sub-tile operands are loaded unconditionally (clamped rows) one sub-tile ahead, and only stores sit under the row mask:
// the waits are counted and the stores of a tile leave back to back.  Same arithmetic, in the same order, as Epi<>::tile.
template <int EK>
__device__ __forceinline__ void wide_epilogue(const Epi<EK>& ep, const f32x4 (&acc)[8][4], float* st, int m_w, int n_w, int lane) {
    const EpiDesc& d = ep.d;
    const int fr = lane & 15, g = lane >> 4;
    auto stage = [&](int i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[(4 * g + r) * EP + 16 * j + fr] = acc[i][j][r];
    };
    if constexpr (EK == E_F32 || EK == E_BF16 || EK == E_BF16_GELU || EK == E_GELU_GRAD) {
        // Row-major outputs.  A store instruction writes WHOLE 128-byte lines: fp32: 4 rows x 256 bytes (lane -> row 4 q + (lane >> 4),
        // 4 columns), bf16: 8 rows x 128 bytes (lane -> row 8 q + (lane >> 3), 8 columns).  With Epi<>::tile's map (a lane owns 16
        // columns of one row: an instruction writes 16-byte pieces 64 bytes apart) a line is completed by four instructions, and once
        // the stores leave back to back lines are evicted half written: measured 67 us per tile of 256 KB instead of 20.
        // N is a multiple of 256 here: no column tail.
        constexpr bool F32O = EK == E_F32;
        constexpr int NQ = F32O ? 4 : 2, RQ = 16 / NQ, CW = F32O ? 4 : 8;      // instructions per sub-tile, rows per instruction, columns per lane
        const int rl = F32O ? (lane >> 4) : (lane >> 3), cl = F32O ? (lane & 15) * 4 : (lane & 7) * 8;
        const int n = n_w + cl;
        f32x4 b4[CW / 4];
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) b4[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (d.bias) {
#pragma unroll
            for (int q = 0; q < CW / 4; ++q) b4[q] = *(const f32x4*)(d.bias + n + 4 * q);
        }
        const bool scatter = (EK == E_F32 || EK == E_BF16) && d.rowidx != nullptr;
        // (compile-time variants for the two uniform run-time conditions, so that every load of a variant is unconditional)
        // Load order: the scatter rows of all eight sub-tiles first; the per-sub-tile operand (residual / pre-activation) of
        // sub-tile i + 1 BEFORE the stores of sub-tile i -- VMEM operations retire in order, so a load issued behind a store is
        // waited for together with that store's acknowledgement.
        auto body = [&](auto scat, auto has_aux) {
            constexpr bool OPL = decltype(has_aux)::value || EK == E_GELU_GRAD;       // a per-sub-tile operand is loaded
            constexpr bool SC = decltype(scat)::value;
            [[maybe_unused]] int dstv[3][NQ];                 // scatter rows of sub-tiles i, i + 1, i + 2 (ring; loaded two ahead)
            auto rows = [&](int i) {
                if constexpr (SC) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) dstv[i % 3][q] = d.rowidx[min(m_w + 16 * i + RQ * q + rl, d.M - 1)];
                }
            };
            rows(0); rows(1);
            auto offs = [&](int i, long (&off)[NQ], bool (&ok)[NQ]) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int m = m_w + 16 * i + RQ * q + rl;
                    int dst = min(m, d.M - 1);
                    if constexpr (SC) dst = dstv[i % 3][q];
                    ok[q] = m < d.M && dst >= 0;
                    off[q] = (long)max(dst, 0) * d.ld + n;
                }
            };
            [[maybe_unused]] f32x4 a[2][NQ];
            [[maybe_unused]] uint4 pv[2][NQ];
            auto opload = [&](int i) {
                if constexpr (OPL) {
                    long off[NQ];
                    bool ok[NQ];
                    offs(i, off, ok);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        if constexpr (EK == E_F32) a[i & 1][q] = *(const f32x4*)((const float*)d.aux + off[q]);
                        else pv[i & 1][q] = *(const uint4*)((const uint16_t*)d.aux + off[q]);
                    }
                }
            };
            opload(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                long off[NQ];
                bool ok[NQ];
                offs(i, off, ok);
                if (i + 2 < 8) rows(i + 2);
                if (i + 1 < 8) opload(i + 1);
                stage(i);
                if constexpr (EK == E_F32) {
                    float* out = (float*)d.out;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        f32x4 v = *(const f32x4*)(st + (RQ * q + rl) * EP + cl);
                        v += b4[0];
                        if constexpr (decltype(has_aux)::value) v += a[i & 1][q];
                        if (ok[q]) *(f32x4*)(out + off[q]) = v;
                    }
                } else {
                    uint16_t* out = (uint16_t*)d.out;
                    [[maybe_unused]] uint16_t* out2 = (uint16_t*)d.aux_out;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        float v[8];
                        *(f32x4*)v = *(const f32x4*)(st + (RQ * q + rl) * EP + cl);
                        *(f32x4*)(v + 4) = *(const f32x4*)(st + (RQ * q + rl) * EP + cl + 4);
                        if constexpr (EK == E_GELU_GRAD) {
                            float hv[8];
                            unpack8(pv[i & 1][q], hv);
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] *= gelu_grad_f(hv[e]);
                            if (ok[q]) *(uint4*)(out + off[q]) = pack8(v);
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] += b4[e >> 2][e & 3];
                            if constexpr (EK == E_BF16_GELU) {
                                float gl[8];
#pragma unroll
                                for (int e = 0; e < 8; ++e) gl[e] = gelu_f(bf2f(f2bf(v[e])));   // GELU of the stored (bf16) pre-activation
                                if (ok[q]) { *(uint4*)(out + off[q]) = pack8(v); *(uint4*)(out2 + off[q]) = pack8(gl); }
                            } else {
                                if (ok[q]) *(uint4*)(out + off[q]) = pack8(v);
                            }
                        }
                    }
                }
            }
        };
        const bool aux = EK == E_F32 && d.aux != nullptr;
        if (scatter) { if (aux) body(std::true_type{}, std::true_type{}); else body(std::true_type{}, std::false_type{}); }
        else { if (aux) body(std::false_type{}, std::true_type{}); else body(std::false_type{}, std::false_type{}); }
    } else if constexpr (EK == E_QKV_HEADS || EK == E_HEADS) {
        if (d.p3 > 64) {                 // lane -> (row lane & 15, 16-column quarter lane >> 4)
            const int nb = n_w + 16 * g;
            f32x4 b4[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            if (d.bias) {
#pragma unroll
                for (int q = 0; q < 4; ++q) b4[q] = *(const f32x4*)(d.bias + nb + 4 * q);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                stage(i);
                heads_item_wide<EK == E_QKV_HEADS, true>(d, st, m_w + 16 * i, n_w, lane, b4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) { stage(i); ep.tile(st, m_w + 16 * i, n_w, lane); }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { stage(i); ep.tile(st, m_w + 16 * i, n_w, lane); }
    }
}

template <int EK>
Epi<EK> make_epi(const swv2_epilogue* e, int M, int N) {
    Epi<EK> ep;
    ep.d.out = e->out; ep.d.bias = e->bias; ep.d.aux = e->aux; ep.d.aux_out = e->aux_out; ep.d.rowidx = e->rowidx;
    ep.d.ld = e->ld; ep.d.M = M; ep.d.N = N;
    ep.d.p0 = e->p[0]; ep.d.p1 = e->p[1]; ep.d.p2 = e->p[2]; ep.d.p3 = e->p[3]; ep.d.p4 = e->p[4];
    ep.d.mg0 = ep.d.mg1 = ep.d.mg2 = 0;
    ep.d.loss_tar = nullptr; ep.d.loss_qw = nullptr; ep.d.loss_part = nullptr; ep.d.loss_resid = nullptr; ep.d.q0 = ep.d.q1 = ep.d.q2 = ep.d.q3 = 0;
    if (EK == E_QKV_HEADS || EK == E_HEADS) put_head_magics(ep.d, head_layout(e->p[0], EK == E_QKV_HEADS ? 3 : 1, e->p[2], e->p[3]));
    if (EK == E_UNPATCH || loss_epi(EK)) { ep.d.mg0 = fdiv_magic((e->p[1] / 4) * (e->p[2] / 4)); ep.d.mg1 = fdiv_magic(e->p[2] / 4); }
    if (loss_epi(EK)) {
        ep.d.loss_tar = e->loss_tar; ep.d.loss_qw = e->loss_qw; ep.d.loss_part = e->loss_part; ep.d.loss_resid = (uint16_t*)e->loss_resid;
        ep.d.q0 = e->q[0]; ep.d.q1 = e->q[1];
        const long nb = M / ((e->p[1] / 4) * (e->p[2] / 4)), plane = (long)e->p[1] * e->p[2];
        // dump areas of the masked lanes: behind the dense prediction, or where the caller says (q[2] floats from `out`: rollouts, where
        // `out` points into a larger tensor); behind the second destination
        ep.d.q2 = e->q[2] ? e->q[2] : (int)(nb * e->p[0] * plane);
        ep.d.q3 = (int)(nb * e->ld * plane);
    }
    return ep;
}

}  // namespace
