// Forecast scores (reference utils/weighted_acc_rmse.py:50-115): latitude-weighted RMSE and anomaly correlation (ACC) of a
// prediction against the verifying analysis, per (sample, channel) plane.  One streaming pass reads prediction, truth and -- for
// ACC -- the climatology once and leaves four weighted sums per plane; torch spends about ten passes and several plane-sized
// temporaries on the same numbers.
//
//   launch 1  score_sums_kernel<CLIM>   8 (12 with clim) B/element   per (plane, slice) partial sums -> workspace
//   launch 2  score_finalize_kernel     one workgroup per channel: folds the slices, RMSE, ACC, the batch means
//
//     S_dd = sum w[h] (p - t)^2      S_pt = sum w[h] p' t'      S_pp = sum w[h] p'^2      S_tt = sum w[h] t'^2
//     p' = p - clim[c][h][w], t' = t - clim[c][h][w]  (p, t themselves without a climatology);  d = p - t is formed from p and t,
//     never as p' - t': RMSE does not depend on the climatology.
//
// Plan and sums: plane_stream.h, with the workgroup index (c * slices + sl) * B + b (the climatology is the shared operand) and
// 4 ceil(v / 256) fma in the thread's own running sum, v = 16-byte vectors of the largest slice (tests/score_reference.py::chain_length).
// A slice without elements stores four zeros.
#include "plane_stream.h"

namespace {

template <bool CLIM>
__device__ __forceinline__ void score_vec(const f32x4 a, const f32x4 b, const f32x4 m, const float q, float (&s)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = a[e] - b[e];
        const float pa = CLIM ? a[e] - m[e] : a[e], ta = CLIM ? b[e] - m[e] : b[e];
        const float qp = q * pa;
        s[0] = fmaf(q * d, d, s[0]);
        s[1] = fmaf(qp, ta, s[1]);
        s[2] = fmaf(qp, pa, s[2]);
        s[3] = fmaf(q * ta, ta, s[3]);
    }
}

template <bool CLIM>
__global__ __launch_bounds__(256) void score_sums_kernel(const float* __restrict__ prd, long prd_bs, const float* __restrict__ tar, long tar_bs,
                                                         const float* __restrict__ clim, const float* __restrict__ w, float* __restrict__ ws,
                                                         int B, int C, int H, int W, int slices) {
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* p = prd + b * prd_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    float s[4];
    if constexpr (CLIM) {
        const float* const op[3] = {p, t, clim + (long)c * plane};
        plane_stream_slice(op, lo, hi, W, w, s, [](const f32x4(&v)[3], float q, float(&a)[4]) { score_vec<true>(v[0], v[1], v[2], q, a); });
    } else {
        const float* const op[2] = {p, t};
        plane_stream_slice(op, lo, hi, W, w, s, [](const f32x4(&v)[2], float q, float(&a)[4]) { score_vec<false>(v[0], v[1], v[1], q, a); });      // (m is not read)
    }
    __shared__ float r[4][4];
    plane_block_stage(s, r);
    if (threadIdx.x == 0) {
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = plane_block_total(r[k]);
        *(f32x4*)(ws + ((size_t)(b * C + c) * slices + sl) * 4) = o;
    }
}

// One workgroup per channel: wave v folds the slice partials of the planes b = v, v + 4, ... (plane_fold_slices) and writes that
// plane's sums, RMSE and ACC; thread 0 then adds the B values of the channel in ascending b for the batch means.
__global__ __launch_bounds__(256) void score_finalize_kernel(const float* __restrict__ ws, int slices, int B, int C, float npix,
                                                             const float* __restrict__ scale, float* __restrict__ sums,
                                                             float* rmse, float* acc,
                                                             float* __restrict__ rmse_mean, float* __restrict__ acc_mean) {
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += 4) {
        const size_t pl = (size_t)b * C + c;
        f32x4 a;
        plane_fold_slices<1>((const f32x4*)ws, pl, slices, lane, &a);
        if (lane == 0) {
            *(f32x4*)(sums + pl * 4) = a;
            rmse[pl] = sqrtf(a[0] / npix);
            acc[pl] = a[1] / sqrtf(a[2] * a[3]);           // 0 / 0 = NaN in this plane only, as in torch
        }
    }
    __syncthreads();                                       // the plane values above are this workgroup's own global stores
    if (threadIdx.x == 0) {
        float sr = 0.f, sa = 0.f;
        for (int b = 0; b < B; ++b) { sr += rmse[(size_t)b * C + c]; sa += acc[(size_t)b * C + c]; }
        sr /= (float)B;
        rmse_mean[c] = scale ? sr * scale[c] : sr;
        acc_mean[c] = sa / (float)B;
    }
}

}  // namespace

extern "C" int swv2_score_slices(int planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    return plane_slices(planes);
}

extern "C" size_t swv2_score_ws_bytes(int planes, int H, int W) { return plane_ws_bytes(planes, H, W, 4); }

extern "C" int swv2_score_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* clim, const float* w,
                               int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(prd && tar && w && ws, "score_sums: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "score_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "score_sums: W % 4 != 0");
    if (!plane_operands_ok("score_sums", {prd, tar, clim, ws}, {prd_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes,
                           swv2_score_ws_bytes(B * C, H, W), "swv2_score_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const dim3 grid((unsigned)((long)B * C * slices));
    if (clim)
        hipLaunchKernelGGL(score_sums_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, prd, prd_bstride, tar, tar_bstride, clim, w,
                           (float*)ws, B, C, H, W, slices);
    else
        hipLaunchKernelGGL(score_sums_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, prd, prd_bstride, tar, tar_bstride, clim, w,
                           (float*)ws, B, C, H, W, slices);
    SWV2_CHECK_LAUNCH("swv2_score_sums");
    return SWV2_OK;
}

extern "C" int swv2_score_finalize(const void* ws, size_t ws_bytes, int B, int C, int H, int W, const float* scale, float* sums, float* rmse,
                                   float* acc, float* rmse_mean, float* acc_mean, void* stream) {
    SWV2_CHECK_ARG(ws && sums && rmse && acc && rmse_mean && acc_mean, "score_finalize: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "score_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("score_finalize", {ws, sums}, {}, 1, 0, ws_bytes, swv2_score_ws_bytes(B * C, H, W), "swv2_score_ws_bytes"))
        return SWV2_ERR_INVALID;
    hipLaunchKernelGGL(score_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, (const float*)ws, plane_slices((long)B * C), B, C,
                       (float)((long)H * W), scale, sums, rmse, acc, rmse_mean, acc_mean);
    SWV2_CHECK_LAUNCH("swv2_score_finalize");
    return SWV2_OK;
}
