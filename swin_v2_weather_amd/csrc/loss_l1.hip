// Geometric l1 loss (reference utils/losses.py:114-120, 188-240 with p = 1; grids.py:115-117): the latitude-weighted sums of |prd - tar|
// and |tar| per (sample, channel) plane, the [B, C] arithmetic of the loss value, and the gradient d loss / d prd.
//
//   launch 1  l1_sums_kernel       8 B/element   per (plane, slice) partial sums (S0, S1) -> workspace
//   launch 2  l1_finalize_kernel   one workgroup: folds the slices, sums[B C][2]; with chw also the loss and coef[B C]
//   backward  plane_grad_kernel<L1Grad>   8 B/element read, 4 written: dprd = coef[bc] q[h] sign(prd - tar)
//
//     S0 = sum q[h] |p - t|      S1 = sum q[h] |t|      norm = S0 (absolute) or S0 / S1      loss = sum_bc chw[c] norm[b, c]
//     coef[bc] = d loss / d S0[bc] = chw[c] (absolute) or chw[c] / S1[bc]
//
// Plan and sums: plane_stream.h, with the workgroup index plane * slices + sl (only the row weights are shared) and 4 ceil(v / 256) fma
// in the thread's own running sum, v = 16-byte vectors of the largest slice (tests/l1_reference.py::chain_length).  Per element the
// compiler spends one subtraction, two sign-bit clears and ONE packed fma for both sums (|x| would be a free source modifier of a scalar
// fma; the packed form has none): four vector ALU instructions per 8 bytes read, a tenth of what the read stream leaves room for.
// A slice without elements stores two zeros.
#include "plane_stream.h"

namespace {

__device__ __forceinline__ void l1_vec(const f32x4 a, const f32x4 b, const float q, float (&s)[2]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s[0] = fmaf(q, fabsf(a[e] - b[e]), s[0]);
        s[1] = fmaf(q, fabsf(b[e]), s[1]);
    }
}

__global__ __launch_bounds__(256) void l1_sums_kernel(const float* __restrict__ prd, long prd_bs, const float* __restrict__ tar, long tar_bs,
                                                      const float* __restrict__ w, float* __restrict__ ws, int C, int H, int W, int slices) {
    const int pl = blockIdx.x / slices, sl = blockIdx.x - pl * slices, b = pl / C, c = pl - b * C;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* const op[2] = {prd + b * prd_bs + (long)c * plane, tar + b * tar_bs + (long)c * plane};
    float s[2];
    plane_stream_slice(op, lo, hi, W, w, s, [](const f32x4(&v)[2], float q, float(&a)[2]) { l1_vec(v[0], v[1], q, a); });
    __shared__ float r[2][4];
    plane_block_stage(s, r);
    if (threadIdx.x == 0) *(float2*)(ws + ((size_t)pl * slices + sl) * 2) = make_float2(plane_block_total(r[0]), plane_block_total(r[1]));
}

// One workgroup of L1_FIN_WAVES waves: wave v folds the slice partials of the planes v, v + 16, ... in ascending order
// (plane_fold_slices), writes that plane's sums and -- with chw -- its coef, and keeps the running sum of its planes' terms chw[c] norm;
// the waves' sums meet in LDS and thread 0 adds them as a fixed binary tree, (w_i + w_{i+8}), then + 4, + 2, + 1.  Every lane of a wave
// holds the same values after the butterfly, so the running sum needs no second one.  (Sixteen waves, not four: a plane costs a wave two
// dependent memory round trips, and with four waves the 146 planes of the training shape took 44 us.)
constexpr int L1_FIN_WAVES = 16;

__global__ __launch_bounds__(64 * L1_FIN_WAVES) void l1_finalize_kernel(const float* __restrict__ ws, int slices, int planes, int C,
                                                                        const float* __restrict__ chw, int absolute,
                                                                        float* __restrict__ sums, float* __restrict__ loss,
                                                                        float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    float acc = 0.f;
    for (int pl = threadIdx.x >> 6; pl < planes; pl += L1_FIN_WAVES) {
        float a[2];
        plane_fold_slices<2>(ws, (size_t)pl, slices, lane, a);
        if (lane == 0) *(float2*)(sums + (size_t)pl * 2) = make_float2(a[0], a[1]);
        if (chw) {
            const float cw = chw[pl % C];
            const float cf = absolute ? cw : cw / a[1];
            acc += absolute ? cw * a[0] : cw * (a[0] / a[1]);
            if (lane == 0) coef[pl] = cf;
        }
    }
    if (!chw) return;                                      // (uniform: no thread reaches the barrier)
    __shared__ float r[L1_FIN_WAVES];
    if (lane == 0) r[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[L1_FIN_WAVES];
#pragma unroll
        for (int i = 0; i < L1_FIN_WAVES; ++i) t[i] = r[i];
#pragma unroll
        for (int s = L1_FIN_WAVES / 2; s > 0; s >>= 1)
#pragma unroll
            for (int i = 0; i < s; ++i) t[i] += t[i + s];
        *loss = t[0];
    }
}

// The element rule of plane_grad_kernel, c = coef[bc] q[h].  The sign comes from the two comparisons, never from the rounded
// difference: exact whatever the denormal mode, 0 where p == t (as torch.abs differentiates) and where either is NaN.
struct L1Grad {
    static __device__ __forceinline__ float grad(float c, float p, float t) { return p > t ? c : (p < t ? -c : 0.f); }
};

}  // namespace

extern "C" size_t swv2_l1_ws_bytes(int planes, int H, int W) { return plane_ws_bytes(planes, H, W, 2); }

extern "C" int swv2_l1_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* w, int B, int C, int H, int W,
                            void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(prd && tar && w && ws, "l1_sums: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "l1_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "l1_sums: W % 4 != 0");
    if (!plane_operands_ok("l1_sums", {prd, tar, ws}, {prd_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes, swv2_l1_ws_bytes(B * C, H, W),
                           "swv2_l1_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    hipLaunchKernelGGL(l1_sums_kernel, dim3((unsigned)((long)B * C * slices)), dim3(256), 0, (hipStream_t)stream, prd, prd_bstride, tar,
                       tar_bstride, w, (float*)ws, C, H, W, slices);
    SWV2_CHECK_LAUNCH("swv2_l1_sums");
    return SWV2_OK;
}

extern "C" int swv2_l1_finalize(const void* ws, size_t ws_bytes, int B, int C, int H, int W, const float* chw, int absolute, float* sums,
                                float* loss, float* coef, void* stream) {
    SWV2_CHECK_ARG(ws && sums && (!chw || (loss && coef)), "l1_finalize: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "l1_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("l1_finalize", {ws}, {}, 1, 0, ws_bytes, swv2_l1_ws_bytes(B * C, H, W), "swv2_l1_ws_bytes")) return SWV2_ERR_INVALID;
    SWV2_CHECK_ARG(((uintptr_t)sums & 7) == 0, "l1_finalize: sums not 8-byte aligned");
    hipLaunchKernelGGL(l1_finalize_kernel, dim3(1), dim3(64 * L1_FIN_WAVES), 0, (hipStream_t)stream, (const float*)ws, plane_slices((long)B * C), B * C, C,
                       chw, absolute, sums, loss, coef);
    SWV2_CHECK_LAUNCH("swv2_l1_finalize");
    return SWV2_OK;
}

extern "C" int swv2_l1_grad(const float* prd, const float* tar, const float* quad_w, const float* coef, float* dprd, int BC, int H, int W,
                            void* stream) {
    return plane_grad_launch<L1Grad>("l1_grad", prd, tar, quad_w, coef, dprd, BC, H, W, stream);
}
