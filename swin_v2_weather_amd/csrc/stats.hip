// Dataset statistics: the running sums behind global_means / global_stds / time_diff_stds / time_means (the four files every config of
// config/swin.yaml names), accumulated slab by slab while the year files stream through the device (utils/dataset_stats.py).
//
//   launch per slab  stats_accumulate_kernel<PREV>  8 (slab + prev) + 16 (tsum read-modify-write) B/element
//   launch at end    stats_fold_kernel              one wave per channel: folds the slice partials in a fixed order
//                    stats_time_means_kernel        time_means = (float)(pivot + tsum / T)
//
//     x' = (double)x - pivot[c]      d = (double)x - (double)prev      (both differences of two fp32 values, formed in fp64)
//     tsum[c][i][j] += x'            part[c][slice] += (sum x', sum x'^2, sum d, sum d^2, number of non-finite x, 0)
//
// fp64 and a pivot: a geopotential-like channel (mean 2e5, std 3e3) loses its variance in a one-pass fp32 sum; shifted by a value near
// the mean and summed in fp64 the one-pass form S2 / N - (S1 / N)^2 cancels nothing that matters.
//
// Plan (swv2_stats_slices, the rule of swv2_score_slices): slices = C >= 2048 ? 1 : 2048 / C workgroups of 256 threads per channel,
// slice sl covering the elements [plane * sl / slices / 4 * 4, plane * (sl + 1) / slices / 4 * 4) of the flattened plane (the last one
// to the end; plane = H W, a multiple of 4).  Every tsum element and every part entry has ONE owner and the slabs are serialised on
// the stream: no atomics, nothing depends on arrival order, two runs on the same inputs agree bit for bit.  first != 0 stores
// instead of adding (tsum and part alike), so the caller never zeroes anything.
//
// Sums: on its way into a channel's sum a term of one slab passes through at most
//     4 ceil(v / 256)   the thread's own running sum (fma), v = 16-byte vectors of the largest slice
//     6                 wave64 butterfly
//     2                 the four waves through LDS, (w0 + w1) + (w2 + w3)
//     1                 the addition into part[c][slice] (one per slab: T of them over a run)
//     ceil(slices / 64) the lane's running sum over the slice partials in swv2_stats_finalize (slices sl = lane, lane + 64, ...)
//     6                 wave64 butterfly
// fp64 additions (tests/stats_reference.py::chain_length states the same count).
#include "common.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int STATS_MAX_BLOCKS = 2048;        // one round at 8 workgroups per CU, as swv2_score_sums

__host__ __device__ inline int stats_slices(long C) { return C >= STATS_MAX_BLOCKS ? 1 : (int)(STATS_MAX_BLOCKS / C); }

__device__ __forceinline__ void slice_range(uint32_t plane, int sl, int slices, uint32_t& lo, uint32_t& hi) {
    lo = (uint32_t)((uint64_t)plane * sl / slices) / 4 * 4;
    hi = (sl + 1 == slices) ? plane : (uint32_t)((uint64_t)plane * (sl + 1) / slices) / 4 * 4;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one 16-byte vector of the slab: 4 elements into the thread's running sums and into their tsum slots (two paired fp64 accesses)
template <bool PREV>
__device__ __forceinline__ void stats_vec(const f32x4 x, const f32x4 pv, const f64x2 t0, const f64x2 t1, const double pivot, const bool first,
                                          double* ts, double (&s)[5]) {
    double xs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xs[e] = (double)x[e] - pivot;
        s[0] += xs[e];
        s[1] = fma(xs[e], xs[e], s[1]);
        if (PREV) {
            const double d = (double)x[e] - (double)pv[e];
            s[2] += d;
            s[3] = fma(d, d, s[3]);
        }
        s[4] += (__float_as_uint(x[e]) & 0x7f800000u) == 0x7f800000u ? 1.0 : 0.0;         // Inf or NaN
    }
    f64x2 o0 = {xs[0], xs[1]}, o1 = {xs[2], xs[3]};
    if (!first) { o0 += t0; o1 += t1; }
    *(f64x2*)ts = o0;
    *(f64x2*)(ts + 2) = o1;
}

template <bool PREV>
__global__ __launch_bounds__(256) void stats_accumulate_kernel(const float* __restrict__ slab, const float* __restrict__ prev,
                                                               const double* __restrict__ pivot, double* __restrict__ tsum,
                                                               double* __restrict__ part, int H, int W, int slices, int first) {
    const int c = blockIdx.x / slices, sl = blockIdx.x - c * slices;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30, a multiple of 4 (checked by the host)
    uint32_t lo, hi;
    slice_range(plane, sl, slices, lo, hi);
    const float* x = slab + (size_t)c * plane;
    const float* p = PREV ? prev + (size_t)c * plane : nullptr;
    double* ts = tsum + (size_t)c * plane;
    const double pv = pivot[c];
    const bool fst = first != 0;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f64x2 zero2 = {0.0, 0.0};
    // two independent 16-byte loads of each fp32 operand and four of tsum in flight per thread
    uint32_t i = lo + threadIdx.x * 4;
    for (; i + 1024 < hi; i += 2 * 1024) {
        f32x4 a[2], b[2];
        f64x2 t[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a[u] = *(const f32x4*)(x + i + u * 1024);
            b[u] = PREV ? *(const f32x4*)(p + i + u * 1024) : zero;
            t[u][0] = fst ? zero2 : *(const f64x2*)(ts + i + u * 1024);
            t[u][1] = fst ? zero2 : *(const f64x2*)(ts + i + u * 1024 + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) stats_vec<PREV>(a[u], b[u], t[u][0], t[u][1], pv, fst, ts + i + u * 1024, s);
    }
    for (; i < hi; i += 1024) {
        const f32x4 a = *(const f32x4*)(x + i);
        const f32x4 b = PREV ? *(const f32x4*)(p + i) : zero;
        const f64x2 t0 = fst ? zero2 : *(const f64x2*)(ts + i), t1 = fst ? zero2 : *(const f64x2*)(ts + i + 2);
        stats_vec<PREV>(a, b, t0, t1, pv, fst, ts + i, s);
    }
    __shared__ double r[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        s[k] = wave_sum_f64(s[k]);
        if ((threadIdx.x & 63) == 0) r[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // the one owner of part[c][sl]
        double* o = part + (size_t)blockIdx.x * 6;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double v = (r[k][0] + r[k][1]) + (r[k][2] + r[k][3]);
            o[k] = fst ? v : o[k] + v;
        }
        if (fst) o[5] = 0.0;                                  // the spare
    }
}

// One wave per channel: lane l adds the slices l, l + 64, ... in ascending order, then the butterfly.
__global__ __launch_bounds__(64) void stats_fold_kernel(const double* __restrict__ part, int slices, double* __restrict__ folded) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int sl = lane; sl < slices; sl += 64) {
        const double* q = part + ((size_t)c * slices + sl) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += q[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = wave_sum_f64(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) folded[(size_t)c * 6 + k] = a[k];
    }
}

// Workgroup (channel, slice) of the accumulate plan: time_means = (float)(pivot + tsum / T).
__global__ __launch_bounds__(256) void stats_time_means_kernel(const double* __restrict__ tsum, const double* __restrict__ pivot, double T,
                                                               float* __restrict__ tm, int H, int W, int slices) {
    const int c = blockIdx.x / slices, sl = blockIdx.x - c * slices;
    const uint32_t plane = (uint32_t)H * W;
    uint32_t lo, hi;
    slice_range(plane, sl, slices, lo, hi);
    const double* ts = tsum + (size_t)c * plane;
    float* o = tm + (size_t)c * plane;
    const double pv = pivot[c];
    for (uint32_t i = lo + threadIdx.x * 4; i < hi; i += 1024) {
        const f64x2 t0 = *(const f64x2*)(ts + i), t1 = *(const f64x2*)(ts + i + 2);
        const f32x4 v = {(float)(pv + t0[0] / T), (float)(pv + t0[1] / T), (float)(pv + t1[0] / T), (float)(pv + t1[1] / T)};
        *(f32x4*)(o + i) = v;
    }
}

inline bool stats_shape_ok(int C, int H, int W) {
    return C > 0 && H > 0 && W > 0 && (long)C < (1L << 31) / STATS_MAX_BLOCKS && (long)H * W < (1L << 30);
}

}  // namespace

extern "C" int swv2_stats_slices(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return stats_slices(C);
}

extern "C" size_t swv2_stats_ws_bytes(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)C * stats_slices(C) * 6 * sizeof(double);
}

extern "C" int swv2_stats_accumulate(const float* slab, const float* prev, const double* pivot, double* tsum, void* part, size_t part_bytes,
                                     int C, int H, int W, int first, void* stream) {
    SWV2_CHECK_ARG(slab && pivot && tsum && part, "stats_accumulate: null pointer");
    SWV2_CHECK_ARG(stats_shape_ok(C, H, W), "stats_accumulate: bad shape (C, H, W > 0, C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((long)H * W % 4 == 0, "stats_accumulate: H * W % 4 != 0");
    SWV2_CHECK_ARG((((uintptr_t)slab | (uintptr_t)prev | (uintptr_t)tsum) & 15) == 0 && (((uintptr_t)pivot | (uintptr_t)part) & 7) == 0,
                   "stats_accumulate: pointer not aligned (slab, prev, tsum: 16 bytes; pivot, part: 8)");
    SWV2_CHECK_ARG(part_bytes >= swv2_stats_ws_bytes(C, H, W), "stats_accumulate: workspace too small (swv2_stats_ws_bytes)");
    const int slices = stats_slices(C);
    const dim3 grid((unsigned)((long)C * slices));
    if (prev)
        hipLaunchKernelGGL(stats_accumulate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, slab, prev, pivot, tsum, (double*)part, H, W,
                           slices, first);
    else
        hipLaunchKernelGGL(stats_accumulate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, slab, prev, pivot, tsum, (double*)part, H, W,
                           slices, first);
    SWV2_CHECK_LAUNCH("swv2_stats_accumulate");
    return SWV2_OK;
}

extern "C" int swv2_stats_finalize(const void* part, size_t part_bytes, const double* tsum, const double* pivot, int C, int H, int W, long T,
                                   double* folded, float* time_means, void* stream) {
    SWV2_CHECK_ARG(part && tsum && pivot && folded && time_means, "stats_finalize: null pointer");
    SWV2_CHECK_ARG(stats_shape_ok(C, H, W), "stats_finalize: bad shape (C, H, W > 0, C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((long)H * W % 4 == 0, "stats_finalize: H * W % 4 != 0");
    SWV2_CHECK_ARG(T > 0, "stats_finalize: T <= 0 (no slab was accumulated)");
    SWV2_CHECK_ARG((((uintptr_t)tsum | (uintptr_t)time_means) & 15) == 0 && (((uintptr_t)pivot | (uintptr_t)part | (uintptr_t)folded) & 7) == 0,
                   "stats_finalize: pointer not aligned (tsum, time_means: 16 bytes; pivot, part, folded: 8)");
    SWV2_CHECK_ARG(part_bytes >= swv2_stats_ws_bytes(C, H, W), "stats_finalize: workspace too small (swv2_stats_ws_bytes)");
    const int slices = stats_slices(C);
    hipLaunchKernelGGL(stats_fold_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, (const double*)part, slices, folded);
    SWV2_CHECK_LAUNCH("swv2_stats_finalize (fold)");
    hipLaunchKernelGGL(stats_time_means_kernel, dim3((unsigned)((long)C * slices)), dim3(256), 0, (hipStream_t)stream, tsum, pivot, (double)T,
                       time_means, H, W, slices);
    SWV2_CHECK_LAUNCH("swv2_stats_finalize (time means)");
    return SWV2_OK;
}
