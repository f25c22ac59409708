// The plan of the plane-streaming kernels, stated once: forecast scores (score.hip), dataset statistics (stats.hip), order statistics
// (quantile.hip), ensemble scores (ensemble.hip), the l1 loss (loss_l1.hip); swv2_loss_sums (rowops.hip) takes its slice count from here.  Each of them reads
// `planes` planes of H x W fp32 values once (planes = B * C, or C for the statistics) and leaves a few numbers per plane.
//
// Slices.  A plane is cut into  slices = planes >= 2048 ? 1 : 2048 / planes  pieces, one workgroup of 256 threads each: at most 2048
// workgroups, one round at 8 per CU (7 .. 56 slices at 146 planes all ran swv2_loss_sums at 4.5 TB/s: the read stream is the bound).
// Slice sl covers the elements [plane_size * sl / slices / 4 * 4, plane_size * (sl + 1) / slices / 4 * 4) of the flattened plane, the last
// one to the end: every bound is a multiple of 4 elements, so a thread's 16-byte vector never straddles one.  A slice without elements
// is legal (a plane of fewer than 4 * slices elements has them) and stores zeros.  tests/plane_reference.py mirrors both rules.
//
// Workgroup index.  (c * slices + sl) * B + b where a per-channel operand is shared (the climatology of score.hip, the row weights of
// ensemble.hip): the B workgroups that read the same piece of it are neighbours in launch order, so it comes from HBM once and from
// the memory-side cache afterwards.  plane * slices + sl where nothing is shared (stats.hip, quantile.hip) or the row weights only (loss_l1.hip).
//
// Sums.  No float atomics and no pre-zeroed output: every partial sum has ONE owner, and the order of the additions is fixed by the
// plan alone, so two runs on the same inputs agree bit for bit.  On its way into a plane's sum a term passes through
//     the thread's own running sum over its vectors of the slice (each kernel states its own count)
//     6                  wave64 butterfly                                                     plane_block_stage
//     2                  the four waves through LDS, (w0 + w1) + (w2 + w3), by thread 0       plane_block_total
//     ceil(slices / 64)  the lane's running sum over the slice partials, sl = lane, lane + 64, ...   plane_fold_slices
//     6                  wave64 butterfly
// additions in the format of the sums (fp32; fp64 in stats.hip).  The chain_length of each tests/*_reference.py states the same count.
// (quantile.hip counts with integer atomics, which no order can change, and uses the slices only.)
#pragma once
#include <initializer_list>

#include "common.h"

constexpr int PLANE_MAX_BLOCKS = 2048;

__host__ __device__ inline int plane_slices(long planes) { return planes >= PLANE_MAX_BLOCKS ? 1 : (int)(PLANE_MAX_BLOCKS / planes); }

// element range [lo, hi) of slice sl of a plane of `plane` < 2^30 elements (a multiple of 4)
__device__ __forceinline__ void plane_slice_range(uint32_t plane, int sl, int slices, uint32_t& lo, uint32_t& hi) {
    lo = (uint32_t)((uint64_t)plane * sl / slices) / 4 * 4;
    hi = (sl + 1 == slices) ? plane : (uint32_t)((uint64_t)plane * (sl + 1) / slices) / 4 * 4;
}

// The fp64 butterfly.  Its own name on purpose: an overload wave_sum(double) declared inside a file's anonymous namespace would hide
// wave_sum(float) there and turn every fp32 butterfly of that file into an fp64 one.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the butterfly of one value of the kinds the partial sums are kept in: a float, a double, or four floats as one 16-byte vector
__device__ __forceinline__ float plane_wave_sum(float v) { return wave_sum(v); }
__device__ __forceinline__ double plane_wave_sum(double v) { return wave_sum_f64(v); }
__device__ __forceinline__ f32x4 plane_wave_sum(f32x4 v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    return v;
}

// Workgroup reduction of N running sums, first half, all 256 threads: the butterfly, then wave v's sums into r[k][v]; ends in the
// barrier.  Second half, the owner alone (inside its `if (threadIdx.x == 0)`, so nobody else pays for it): plane_block_total(r[k]).
template <class T, int N>
__device__ __forceinline__ void plane_block_stage(T (&s)[N], T (&r)[N][4]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        s[k] = plane_wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) r[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
}

template <class T>
__device__ __forceinline__ T plane_block_total(const T (&r)[4]) { return (r[0] + r[1]) + (r[2] + r[3]); }

// Slice fold by one wave: lane l adds the partials (N values of type V per slice) of the slices l, l + 64, ... of plane pl in ascending
// order, then the butterfly; every lane ends with the plane's sums in a[0 .. N).
template <int N, class V>
__device__ __forceinline__ void plane_fold_slices(const V* __restrict__ part, size_t pl, int slices, int lane, V* a) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = V{};
    for (int sl = lane; sl < slices; sl += 64) {
        const V* q = part + (pl * slices + sl) * N;
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += q[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = plane_wave_sum(a[k]);
}

// ---- host side ----------------------------------------------------------------------------
// planes * slices fits the 32-bit grid index, an element index fits 30 bits
inline bool plane_shape_ok(long planes, int H, int W) {
    return planes > 0 && H > 0 && W > 0 && planes < (1L << 31) / PLANE_MAX_BLOCKS && (long)H * W < (1L << 30);
}

// The operands of an entry point that reads blocks of planes in place ([B, C, H, W] with contiguous planes, sample b at p + b * bstride):
// the `vec` pointers are read or written as 16-byte vectors (null: absent), a batch stride keeps them so and -- unless B == 1, where it
// is never used -- steps over the `span` = C * H * W elements of a sample, and the workspace holds what `ws_fn` asks for.
inline bool plane_operands_ok(const char* who, std::initializer_list<const void*> vec, std::initializer_list<long> bstrides, int B, long span,
                              size_t ws_bytes, size_t ws_need, const char* ws_fn) {
    for (const void* p : vec)
        if ((uintptr_t)p & 15) return swv2_set_error("%s: pointer not 16-byte aligned", who), false;
    for (long s : bstrides)
        if (s % 4 != 0) return swv2_set_error("%s: batch stride not a multiple of 4", who), false;
    for (long s : bstrides)
        if (B != 1 && s < span) return swv2_set_error("%s: batch stride smaller than the C planes of a sample", who), false;
    if (ws_bytes < ws_need) return swv2_set_error("%s: workspace too small (%s)", who, ws_fn), false;
    return true;
}
