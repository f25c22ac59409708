// Geometric l2 loss (reference utils/losses.py:188-232, grids.py:115-117): the latitude-weighted sums of (prd - tar)^2 and tar^2 per
// (sample, channel) plane, the [B, C] arithmetic of the loss value, and the gradient d loss / d prd.
//
//   launch 1  loss_sums_kernel            8 B/element   per (plane, slice) partial sums (S0, S1) -> workspace
//   launch 2  loss_fold_kernel            one wave per plane: folds the slices, sums[B C][2]
//   launch 3  loss_finalize_kernel        one workgroup: the loss and coef[B C] from sums (also from the head epilogue's sums, below)
//   backward  plane_grad_kernel<L2Grad>   8 B/element read, 4 written: dprd = coef[bc] q[h] (prd - tar)
//
//     S0 = sum q[h] (p - t)^2      S1 = sum q[h] t^2      (coef from loss_finalize_kernel: the chain rule of the chosen l2 variant)
//
// Plan and sums: plane_stream.h, with the workgroup index plane * slices + sl (only the row weights are shared) and 4 ceil(v / 256) fma
// in the thread's own running sum, v = 16-byte vectors of the largest slice.  S0 and S1 are the fma chains of S_dd and S_tt of score.hip
// without a climatology, over the same plan: the same bits (tests/test_l2_loss_gpu.py).  A slice without elements stores two zeros.
// In training the sums usually come from the head GEMM's epilogue instead (gemm.hip, Epi<E_UNPATCH_LOSS>; the last two kernels here).
#include "plane_stream.h"

namespace {

__device__ __forceinline__ void l2_vec(const f32x4 a, const f32x4 b, const float q, float (&s)[2]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = a[e] - b[e];
        s[0] = fmaf(q * d, d, s[0]);
        s[1] = fmaf(q * b[e], b[e], s[1]);
    }
}

__global__ __launch_bounds__(256) void loss_sums_kernel(const float* __restrict__ prd, const float* __restrict__ tar,
                                                        const float* __restrict__ qw, float* __restrict__ ws, int H, int W, int slices) {
    const int pl = blockIdx.x / slices, sl = blockIdx.x - pl * slices;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* const op[2] = {prd + (size_t)pl * plane, tar + (size_t)pl * plane};
    float s[2];
    plane_stream_slice(op, lo, hi, W, qw, s, [](const f32x4(&v)[2], float q, float(&a)[2]) { l2_vec(v[0], v[1], q, a); });
    __shared__ float r[2][4];
    plane_block_stage(s, r);
    if (threadIdx.x == 0) *(float2*)(ws + (size_t)blockIdx.x * 2) = make_float2(plane_block_total(r[0]), plane_block_total(r[1]));
}

// wave v of workgroup g folds the slice partials of plane 4 g + v (plane_fold_slices) and writes that plane's two sums
__global__ __launch_bounds__(256) void loss_fold_kernel(const float* __restrict__ ws, int slices, int planes, float* __restrict__ sums) {
    const int pl = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pl >= planes) return;
    float a[2];
    plane_fold_slices<2>(ws, (size_t)pl, slices, lane, a);
    if (lane == 0) *(float2*)(sums + (size_t)pl * 2) = make_float2(a[0], a[1]);
}

// the element rule of plane_grad_kernel, c = coef[bc] q[h]
struct L2Grad {
    static __device__ __forceinline__ float grad(float c, float p, float t) { return c * (p - t); }
};

// loss = sum_{b,c} chw[c] f(S0 / S1)  (relative; S0 alone when absolute; f = sqrt unless squared) and the coefficient
// the backward kernel multiplies in: coef[bc] = 2 d loss / d S0[bc].  One workgroup; replaces the half dozen elementwise /
// reduction launches (and as many again in their autograd) that torch spent on this [B, C] tensor (losses.py:188-232).
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ sums, int layers, const float* __restrict__ chw,
                                                            int BC, int C, int absolute, int squared,
                                                            float* __restrict__ loss, float* __restrict__ coef) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < BC; i += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int l = 0; l < layers; ++l) { s0 += sums[((size_t)l * BC + i) * 2]; s1 += sums[((size_t)l * BC + i) * 2 + 1]; }
        const float w = chw[i % C];
        const float den = absolute ? 1.f : s1;
        const float r = s0 / den;
        float f, df;                                    // f(r), f'(r)
        if (squared) { f = r; df = 1.f; } else { f = sqrtf(r); df = 0.5f / f; }
        acc += w * f;
        coef[i] = 2.f * w * df / den;
    }
    acc = wave_sum(acc);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (red[0] + red[1]) + (red[2] + red[3]);
}

// per-group partial sums of the head epilogue (gemm.hip, Epi<E_UNPATCH_LOSS>: part[g][slot][Cout][2]) -> sums[j][b][..].  grid =
// (B, SWV2_LOSS_PART_SLICES), 4 sub-slices of 256 threads; thread v < 2 Cout owns one (channel, sum) value and adds the groups
// of its sample, slice and sub-slice in ascending order (coalesced: the 2 Cout values of a group slot are contiguous); the
// sub-slices are combined through LDS in a fixed order.  Slot 1 of the group in front of the sample's first group holds the
// rows of this sample that sit in a group starting in the previous one.
__global__ __launch_bounds__(1024) void loss_part_reduce_kernel(const float* __restrict__ part, int M, int T, int Cout, int Ct,
                                                                int coff, int B, float* __restrict__ sums) {
    const int b = blockIdx.x, j = blockIdx.y, nv = 2 * Cout;
    constexpr int GR = SWV2_LOSS_GROUP_ROWS;
    const int ngroups = (M + GR - 1) / GR;
    const int g_lo = (b * T + GR - 1) / GR, g_hi = min(((b + 1) * T + GR - 1) / GR, ngroups);     // groups whose first row lies in sample b
    constexpr int S = SWV2_LOSS_PART_SLICES;
    const int sub = threadIdx.x >> 8, t = threadIdx.x & 255;
    __shared__ float red[3][256];
    const int g0 = g_lo + ((j - g_lo) % S + S) % S + sub * S;          // first g >= g_lo with g % S == j, then the sub's offset
    const size_t gs = (size_t)2 * nv;                                  // floats per group
    for (int v0 = 0; v0 < nv; v0 += 256) {
        const int v = v0 + t;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (v < nv) {
            int g = g0;
            for (; g + 12 * S < g_hi; g += 16 * S) {
                a0 += part[(size_t)g * gs + v];
                a1 += part[(size_t)(g + 4 * S) * gs + v];
                a2 += part[(size_t)(g + 8 * S) * gs + v];
                a3 += part[(size_t)(g + 12 * S) * gs + v];
            }
            for (; g < g_hi; g += 4 * S) a0 += part[(size_t)g * gs + v];
            if (sub == 0 && b > 0 && g_lo > 0 && (g_lo - 1) % S == j) a1 += part[(size_t)(g_lo - 1) * gs + nv + v];
        }
        const float tot = (a0 + a1) + (a2 + a3);
        if (sub) red[sub - 1][t] = tot;
        __syncthreads();
        if (!sub && v < nv) sums[(((size_t)j * B + b) * Ct + coff) * 2 + v] = ((tot + red[0][t]) + red[1][t]) + red[2][t];
        __syncthreads();
    }
}

// The loss epilogue's weighted residual back in IMAGE layout, scaled: out[b][c][4i+p][4j+q] = coef[b][c] * resid[(b,i,j)][c*16 + p*4 + q]
// (+ add[b][c][..]) -- d loss / d prediction of a rollout step whose head carries a skip connection from an input that needs a
// gradient (swinv2_global.py:799-801 inside helpers.py:26-41).  Workgroup = 16 consecutive patches of one patch row: their residual rows
// (16 x N bf16, contiguous rows) go through LDS, then lane -> (patch, image row p) per channel so that a store instruction writes
// 256 contiguous bytes.  Reads 2 N bytes per patch once; the two-pass plane_grad_kernel reads prediction and target (8 N bytes).
template <int TOK>
__global__ __launch_bounds__(256) void resid_to_image_kernel(const uint16_t* __restrict__ resid, const float* __restrict__ coef,
                                                             const float* __restrict__ add, float* __restrict__ out, int Cout, int H,
                                                             int W, int Cs, int Cadd, int gw) {
    extern __shared__ __attribute__((aligned(16))) uint16_t rs[];
    const int N = Cout * 16, P = N + 8;                    // LDS pitch
    const int RP = SWV2_LOSS_RESID_PITCH(N);               // row pitch of the residual in memory
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * TOK, i = blockIdx.y, b = blockIdx.z;
    const int gh = H >> 2;
    const long m0 = ((long)b * gh + i) * gw + j0;
    const int ntok = min(TOK, gw - j0);
    const int cpr = N / 8;                                 // 16-byte chunks per row
    for (int u = tid; u < ntok * cpr; u += 256) {
        const int t = u / cpr, ch = u - t * cpr;
        *(uint4*)(rs + t * P + 8 * ch) = *(const uint4*)(resid + (m0 + t) * RP + 8 * ch);
    }
    __syncthreads();
    const int t = tid & (TOK - 1);
    const long plane = (long)H * W;
    for (int cp = tid / TOK; cp < Cout * 4; cp += 256 / TOK) {
        const int c = cp >> 2, p = cp & 3;
        if (t >= ntok) continue;
        const uint2 r = *(const uint2*)(rs + t * P + c * 16 + p * 4);
        const float cf = coef[b * Cout + c];
        f32x4 v = {cf * __uint_as_float(r.x << 16), cf * __uint_as_float(r.x & 0xffff0000u), cf * __uint_as_float(r.y << 16),
                   cf * __uint_as_float(r.y & 0xffff0000u)};
        const long pix = (long)(4 * i + p) * W + 4 * (j0 + t);
        if (add) v += *(const f32x4*)(add + ((long)b * Cadd + c) * plane + pix);
        *(f32x4*)(out + ((long)b * Cs + c) * plane + pix) = v;
    }
}

}  // namespace

extern "C" size_t swv2_loss_ws_bytes(int planes, int H, int W) { return plane_ws_bytes(planes, H, W, 2); }

extern "C" int swv2_loss_sums(const float* prd, const float* tar, const float* quad_w, float* sums, int BC, int H, int W, void* ws,
                              size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(prd && tar && quad_w && sums && ws, "loss_sums: null pointer");
    SWV2_CHECK_ARG(plane_shape_ok(BC, H, W), "loss_sums: bad shape (B * C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "loss_sums: W % 4 != 0");
    if (!plane_operands_ok("loss_sums", {prd, tar, ws}, {}, 1, 0, ws_bytes, swv2_loss_ws_bytes(BC, H, W), "swv2_loss_ws_bytes"))
        return SWV2_ERR_INVALID;
    SWV2_CHECK_ARG(((uintptr_t)sums & 7) == 0, "loss_sums: sums not 8-byte aligned");
    const int slices = plane_slices(BC);
    hipLaunchKernelGGL(loss_sums_kernel, dim3((unsigned)((long)BC * slices)), dim3(256), 0, (hipStream_t)stream, prd, tar, quad_w, (float*)ws, H,
                       W, slices);
    hipLaunchKernelGGL(loss_fold_kernel, dim3(cdiv(BC, 4)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, slices, BC, sums);
    SWV2_CHECK_LAUNCH("swv2_loss_sums");
    return SWV2_OK;
}

extern "C" int swv2_loss_part_reduce(const float* part, int M, int T, int B, int Cout, int Ct, int coff, float* sums, void* stream) {
    SWV2_CHECK_ARG(part && sums && M > 0 && T >= SWV2_LOSS_GROUP_ROWS && B > 0 && M == B * T && Cout > 0 && coff >= 0 && coff + Cout <= Ct,
                   "loss_part_reduce: bad argument");
    hipLaunchKernelGGL(loss_part_reduce_kernel, dim3(B, SWV2_LOSS_PART_SLICES), dim3(1024), 0, (hipStream_t)stream, part, M, T, Cout,
                       Ct, coff, B, sums);
    SWV2_CHECK_LAUNCH("swv2_loss_part_reduce");
    return SWV2_OK;
}

extern "C" int swv2_loss_finalize(const float* sums, int layers, const float* chw, int BC, int C, int absolute, int squared, float* loss,
                                  float* coef, void* stream) {
    SWV2_CHECK_ARG(sums && chw && loss && coef && BC > 0 && C > 0 && BC % C == 0 && layers > 0, "loss_finalize: bad argument");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, layers, chw, BC, C, absolute, squared, loss,
                       coef);
    SWV2_CHECK_LAUNCH("swv2_loss_finalize");
    return SWV2_OK;
}

extern "C" int swv2_loss_grad(const float* prd, const float* tar, const float* quad_w, const float* coef, float* dprd,
                              int BC, int H, int W, void* stream) {
    return plane_grad_launch<L2Grad>("loss_grad", prd, tar, quad_w, coef, dprd, BC, H, W, stream);
}

extern "C" int swv2_loss_resid_to_image(const void* resid, const float* coef, const float* add, float* out, int B, int Cout, int H, int W,
                                        int Cs, int Cadd, void* stream) {
    SWV2_CHECK_ARG(resid && coef && out && B > 0 && Cout > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0 && Cs >= Cout && (!add || Cadd >= Cout),
                   "loss_resid_to_image: bad argument");
    SWV2_CHECK_ARG(B <= 65535 && H / 4 <= 65535, "loss_resid_to_image: grid too large");
    SWV2_CHECK_ARG((((uintptr_t)resid | (uintptr_t)out | (uintptr_t)add) & 15) == 0, "loss_resid_to_image: unaligned pointer");
    constexpr int TOK = 16;
    const int gw = W / 4, gh = H / 4;
    const size_t lds = (size_t)TOK * (Cout * 16 + 8) * 2;
    SWV2_CHECK_ARG(lds <= 64 * 1024, "loss_resid_to_image: Cout too large for the staging tile");
    hipLaunchKernelGGL((resid_to_image_kernel<TOK>), dim3(cdiv(gw, TOK), gh, B), dim3(256), lds, (hipStream_t)stream, (const uint16_t*)resid,
                       coef, add, out, Cout, H, W, Cs, Cadd, gw);
    SWV2_CHECK_LAUNCH("swv2_loss_resid_to_image");
    return SWV2_OK;
}
