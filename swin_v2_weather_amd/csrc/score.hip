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
// Plan (swv2_score_slices, the same rule as swv2_loss_sums): slices = planes >= 2048 ? 1 : 2048 / planes workgroups of 256 threads
// per plane, slice sl covering the elements [plane_size * sl / slices / 4 * 4, plane_size * (sl + 1) / slices / 4 * 4) (the last
// one to the end).  A slice without elements stores four zeros.  Workgroup index = (c * slices + sl) * B + b: the B workgroups
// that read the same piece of the climatology are neighbours in launch order, so that piece is fetched from HBM once and
// served from the memory-side cache to the others.
//
// Sums: no atomics and no pre-zeroed output; the order is fixed by the plan alone, so two runs on the same inputs agree bit for
// bit.  On its way into a plane's sum a term passes through at most
//     4 ceil(v / 256)   the thread's own running sum (fma), v = 16-byte vectors of the largest slice
//     6                 wave64 butterfly
//     2                 the four waves through LDS, (w0 + w1) + (w2 + w3)
//     ceil(slices / 64) the lane's running sum over the slice partials in swv2_score_finalize (slices sl = lane, lane + 64, ...)
//     6                 wave64 butterfly
// fp32 additions (tests/score_reference.py::chain_length states the same count).
#include "common.h"

namespace {

constexpr int SCORE_MAX_BLOCKS = 2048;        // one round at 8 workgroups per CU, as swv2_loss_sums

__host__ __device__ inline int score_slices(long planes) { return planes >= SCORE_MAX_BLOCKS ? 1 : (int)(SCORE_MAX_BLOCKS / planes); }

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
    const int b = blockIdx.x % B, cs = blockIdx.x / B, c = cs / slices, sl = cs - c * slices;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    const uint32_t lo = (uint32_t)((uint64_t)plane * sl / slices) / 4 * 4;
    const uint32_t hi = (sl + 1 == slices) ? plane : (uint32_t)((uint64_t)plane * (sl + 1) / slices) / 4 * 4;
    const float* p = prd + b * prd_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    const float* m = CLIM ? clim + (long)c * plane : nullptr;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // four independent 16-byte loads of each operand in flight per thread (loss_sums_kernel: one per iteration ran at 4.2 TB/s)
    uint32_t i = lo + threadIdx.x * 4;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {
        f32x4 a[4], bb[4], mm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *(const f32x4*)(p + i + u * 1024);
            bb[u] = *(const f32x4*)(t + i + u * 1024);
            mm[u] = CLIM ? *(const f32x4*)(m + i + u * 1024) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) score_vec<CLIM>(a[u], bb[u], mm[u], w[(i + u * 1024) / (uint32_t)W], s);
    }
    for (; i < hi; i += 1024) {
        const f32x4 a = *(const f32x4*)(p + i), bb = *(const f32x4*)(t + i);
        const f32x4 mm = CLIM ? *(const f32x4*)(m + i) : zero;
        score_vec<CLIM>(a, bb, mm, w[i / (uint32_t)W], s);      // W % 4 == 0: the 4 elements share a latitude row
    }
    __shared__ float r[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) r[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (r[k][0] + r[k][1]) + (r[k][2] + r[k][3]);
        *(f32x4*)(ws + ((size_t)(b * C + c) * slices + sl) * 4) = o;
    }
}

// One workgroup per channel: wave v folds the slice partials of the planes b = v, v + 4, ... (lane l adds the slices l, l + 64, ...
// in ascending order, then the butterfly) and writes that plane's sums, RMSE and ACC; thread 0 then adds the B values of the channel
// in ascending b for the batch means.
__global__ __launch_bounds__(256) void score_finalize_kernel(const float* __restrict__ ws, int slices, int B, int C, float npix,
                                                             const float* __restrict__ scale, float* __restrict__ sums,
                                                             float* rmse, float* acc,
                                                             float* __restrict__ rmse_mean, float* __restrict__ acc_mean) {
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += 4) {
        const size_t pl = (size_t)b * C + c;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int sl = lane; sl < slices; sl += 64) a += *(const f32x4*)(ws + (pl * slices + sl) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = wave_sum(a[k]);
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

inline bool score_shape_ok(int B, int C, int H, int W) {
    return B > 0 && C > 0 && H > 0 && W > 0 && (long)B * C < (1L << 31) / SCORE_MAX_BLOCKS && (long)H * W < (1L << 30);
}

}  // namespace

extern "C" int swv2_score_slices(int planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    return score_slices(planes);
}

extern "C" size_t swv2_score_ws_bytes(int planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)planes * score_slices(planes) * 4 * sizeof(float);
}

extern "C" int swv2_score_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* clim, const float* w,
                               int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(prd && tar && w && ws, "score_sums: null pointer");
    SWV2_CHECK_ARG(score_shape_ok(B, C, H, W), "score_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "score_sums: W % 4 != 0");
    SWV2_CHECK_ARG((((uintptr_t)prd | (uintptr_t)tar | (uintptr_t)clim | (uintptr_t)ws) & 15) == 0, "score_sums: pointer not 16-byte aligned");
    SWV2_CHECK_ARG(prd_bstride % 4 == 0 && tar_bstride % 4 == 0, "score_sums: batch stride not a multiple of 4");
    const long span = (long)C * H * W;
    SWV2_CHECK_ARG(B == 1 || (prd_bstride >= span && tar_bstride >= span), "score_sums: batch stride smaller than the C planes of a sample");
    SWV2_CHECK_ARG(ws_bytes >= swv2_score_ws_bytes(B * C, H, W), "score_sums: workspace too small (swv2_score_ws_bytes)");
    const int slices = score_slices((long)B * C);
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
    SWV2_CHECK_ARG(score_shape_ok(B, C, H, W), "score_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((((uintptr_t)ws | (uintptr_t)sums) & 15) == 0, "score_finalize: pointer not 16-byte aligned (ws, sums)");
    SWV2_CHECK_ARG(ws_bytes >= swv2_score_ws_bytes(B * C, H, W), "score_finalize: workspace too small (swv2_score_ws_bytes)");
    hipLaunchKernelGGL(score_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, (const float*)ws, score_slices((long)B * C), B, C,
                       (float)((long)H * W), scale, sums, rmse, acc, rmse_mean, acc_mean);
    SWV2_CHECK_LAUNCH("swv2_score_finalize");
    return SWV2_OK;
}
