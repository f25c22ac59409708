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
// Plan and sums: plane_stream.h with planes = C, the workgroup index c * slices + sl and fp64 sums.  Every tsum element and every part
// entry has ONE owner and the slabs are serialised on the stream; first != 0 stores instead of adding (tsum and part alike), so the
// caller never zeroes anything.  The thread's own running sum takes 4 ceil(v / 256) additions, v = 16-byte vectors of the largest
// slice, and between the workgroup reduction and the slice fold a term passes through one more: the addition into part[c][slice],
// once per slab, T of them over a run (tests/stats_reference.py::chain_length).
#include "plane_stream.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));

namespace {

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
    plane_slice_range(plane, sl, slices, lo, hi);
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
    plane_block_stage(s, r);
    if (threadIdx.x == 0) {                                   // the one owner of part[c][sl]
        double* o = part + (size_t)blockIdx.x * 6;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double v = plane_block_total(r[k]);
            o[k] = fst ? v : o[k] + v;
        }
        if (fst) o[5] = 0.0;                                  // the spare
    }
}

// One wave per channel: plane_fold_slices.
__global__ __launch_bounds__(64) void stats_fold_kernel(const double* __restrict__ part, int slices, double* __restrict__ folded) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double a[6];
    plane_fold_slices<6>(part, (size_t)c, slices, lane, a);
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
    plane_slice_range(plane, sl, slices, lo, hi);
    const double* ts = tsum + (size_t)c * plane;
    float* o = tm + (size_t)c * plane;
    const double pv = pivot[c];
    for (uint32_t i = lo + threadIdx.x * 4; i < hi; i += 1024) {
        const f64x2 t0 = *(const f64x2*)(ts + i), t1 = *(const f64x2*)(ts + i + 2);
        const f32x4 v = {(float)(pv + t0[0] / T), (float)(pv + t0[1] / T), (float)(pv + t1[0] / T), (float)(pv + t1[1] / T)};
        *(f32x4*)(o + i) = v;
    }
}

}  // namespace

extern "C" int swv2_stats_slices(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return plane_slices(C);
}

extern "C" size_t swv2_stats_ws_bytes(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)C * plane_slices(C) * 6 * sizeof(double);
}

extern "C" int swv2_stats_accumulate(const float* slab, const float* prev, const double* pivot, double* tsum, void* part, size_t part_bytes,
                                     int C, int H, int W, int first, void* stream) {
    SWV2_CHECK_ARG(slab && pivot && tsum && part, "stats_accumulate: null pointer");
    SWV2_CHECK_ARG(plane_shape_ok(C, H, W), "stats_accumulate: bad shape (C, H, W > 0, C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((long)H * W % 4 == 0, "stats_accumulate: H * W % 4 != 0");
    SWV2_CHECK_ARG((((uintptr_t)pivot | (uintptr_t)part) & 7) == 0, "stats_accumulate: pointer not 8-byte aligned (pivot, part)");
    if (!plane_operands_ok("stats_accumulate", {slab, prev, tsum}, {}, 1, 0, part_bytes, swv2_stats_ws_bytes(C, H, W), "swv2_stats_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices(C);
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
    SWV2_CHECK_ARG(plane_shape_ok(C, H, W), "stats_finalize: bad shape (C, H, W > 0, C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((long)H * W % 4 == 0, "stats_finalize: H * W % 4 != 0");
    SWV2_CHECK_ARG(T > 0, "stats_finalize: T <= 0 (no slab was accumulated)");
    SWV2_CHECK_ARG((((uintptr_t)pivot | (uintptr_t)part | (uintptr_t)folded) & 7) == 0,
                   "stats_finalize: pointer not 8-byte aligned (pivot, part, folded)");
    if (!plane_operands_ok("stats_finalize", {tsum, time_means}, {}, 1, 0, part_bytes, swv2_stats_ws_bytes(C, H, W), "swv2_stats_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices(C);
    hipLaunchKernelGGL(stats_fold_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, (const double*)part, slices, folded);
    SWV2_CHECK_LAUNCH("swv2_stats_finalize (fold)");
    hipLaunchKernelGGL(stats_time_means_kernel, dim3((unsigned)((long)C * slices)), dim3(256), 0, (hipStream_t)stream, tsum, pivot, (double)T,
                       time_means, H, W, slices);
    SWV2_CHECK_LAUNCH("swv2_stats_finalize (time means)");
    return SWV2_OK;
}
