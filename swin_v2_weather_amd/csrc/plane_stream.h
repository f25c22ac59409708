// The plan of the plane-streaming kernels, stated once: forecast scores (score.hip), dataset statistics (stats.hip), order statistics
// (quantile.hip), ensemble scores (ensemble.hip), forecast events (events.hip), the l1 loss (loss_l1.hip), the l2 loss (loss_l2.hip), the
// value range of the int16 packing (packed.hip).  Each of them reads `planes` planes of H x W fp32 values once (planes = B * C, or C for
// the statistics and the packing) and leaves a few numbers per plane.
//
// Slices.  A plane is cut into  slices = planes >= 2048 ? 1 : 2048 / planes  pieces, one workgroup of 256 threads each: at most 2048
// workgroups, one round at 8 per CU (7 .. 56 slices at 146 planes all ran swv2_loss_sums at 4.5 TB/s: the read stream is the bound).
// Slice sl covers the elements [plane_size * sl / slices / 4 * 4, plane_size * (sl + 1) / slices / 4 * 4) of the flattened plane, the last
// one to the end: every bound is a multiple of 4 elements, so a thread's 16-byte vector never straddles one.  A slice without elements
// is legal (a plane of fewer than 4 * slices elements has them) and stores zeros.  tests/plane_reference.py mirrors both rules.
//
// Workgroup index.  (c * slices + sl) * B + b where a per-channel operand is shared (the climatology of score.hip, the base field of
// events.hip, the row weights of ensemble.hip): the B workgroups that read the same piece of it are neighbours in launch order, so it
// comes from HBM once and from the memory-side cache afterwards; plane_shared_index decodes it.  plane * slices + sl where nothing is shared (stats.hip, quantile.hip) or the row weights only (loss_l1.hip,
// loss_l2.hip).  The sum kernels over prediction and truth walk their slice with plane_stream_slice; their gradients are plane_grad_kernel.
//
// Sums.  No float atomics and no pre-zeroed output: every partial sum has ONE owner, and the order of the additions is fixed by the
// plan alone, so two runs on the same inputs agree bit for bit.  On its way into a plane's sum a term passes through
//     the thread's own running sum over its vectors of the slice (each kernel states its own count)
//     6                  wave64 butterfly                                                     plane_block_stage
//     2                  the four waves through LDS, (w0 + w1) + (w2 + w3), by thread 0       plane_block_total
//     ceil(slices / 64)  the lane's running sum over the slice partials, sl = lane, lane + 64, ...   plane_fold_slices
//     6                  wave64 butterfly
// additions in the format of the sums (fp32; fp64 in stats.hip).  The chain_length of each tests/*_reference.py states the same count.
// (quantile.hip counts with integer atomics, which no order can change, and uses the slices only.  The integer counts of ensemble.hip
// and events.hip pass through the same stages -- plane_wave_sum(int), plane_block_total, plane_fold_slices -- in any order they like.)
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

// (b, c, sl) of this workgroup under the shared-operand index (c * slices + sl) * B + b
struct plane_bcs { int b, c, sl; };
__device__ __forceinline__ plane_bcs plane_shared_index(int B, int slices) {
    const int b = blockIdx.x % B, cs = blockIdx.x / B, c = cs / slices;
    return {b, c, cs - c * slices};
}

// The fp64 butterfly.  Its own name on purpose: an overload wave_sum(double) declared inside a file's anonymous namespace would hide
// wave_sum(float) there and turn every fp32 butterfly of that file into an fp64 one.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the butterfly of one value of the kinds the partial sums are kept in: a float, a double, four floats as one 16-byte vector, or an
// integer count
__device__ __forceinline__ float plane_wave_sum(float v) { return wave_sum(v); }
__device__ __forceinline__ int plane_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
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
// order, then the butterfly; every lane ends with the plane's sums in a[0 .. N).  V = int folds one count per slice the same way.
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

// The walk of one thread over the slice [lo, hi) of a plane, for NOPS operands streamed side by side (op[k]: the plane's first element):
// groups of four vectors 1024 elements apart, all 4 NOPS loads issued before the first use (one per iteration ran at 4.2 TB/s), then single vectors.  f(v, q, a) adds the
// terms of one 16-byte vector position to the NS running sums a -- v[k] from operand k, q = w[row] (W % 4 == 0: the 4 elements share a
// latitude row) -- and sees every position once, in ascending order: a sum grows by 4 ceil(vectors / 256) terms.  s: out, the thread's
// sums from zero.  32-bit indices: hi <= plane < 2^30.  (The sums run in an array of this function's own and are handed over at the end:
// summed straight into the caller's array, score_sums_kernel<false> came out with another schedule and ran 5 - 10 % slower.)
template <int NOPS, int NS, class F>
__device__ __forceinline__ void plane_stream_slice(const float* const (&op)[NOPS], uint32_t lo, uint32_t hi, int W, const float* __restrict__ w,
                                                   float (&s)[NS], F&& f) {
    float a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.f;
    uint32_t i = lo + threadIdx.x * 4;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {
        f32x4 v[4][NOPS];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < NOPS; ++k) v[u][k] = *(const f32x4*)(op[k] + i + u * 1024);
#pragma unroll
        for (int u = 0; u < 4; ++u) f(v[u], w[(i + u * 1024) / (uint32_t)W], a);
    }
    for (; i < hi; i += 1024) {
        f32x4 v[NOPS];
#pragma unroll
        for (int k = 0; k < NOPS; ++k) v[k] = *(const f32x4*)(op[k] + i);
        f(v, w[i / (uint32_t)W], a);
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = a[k];
}

// The gradient of a loss whose plane sums carry the row weights: dprd = Rule::grad(coef[bc] * qw[row], p, t) per element.  grid =
// (ceil(plane / 4096), B * C): a workgroup handles 4 x 256 float4 units of one (b, c) plane, all eight loads in flight before the first
// store; 32-bit index arithmetic (the first version did two 64-bit divisions per float4).
template <class Rule>
__global__ __launch_bounds__(256) void plane_grad_kernel(const float* __restrict__ prd, const float* __restrict__ tar,
                                                         const float* __restrict__ qw, const float* __restrict__ coef,
                                                         float* __restrict__ dprd, int H, int W) {
    const int plane = H * W, bc = blockIdx.y;
    const size_t base = (size_t)bc * plane;
    const float cf = coef[bc];
    f32x4 a[4], b[4];
    int idx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        idx[u] = ((blockIdx.x * 4 + u) * 256 + threadIdx.x) * 4;
        const int j = min(idx[u], plane - 4);                        // clamped: unconditional loads
        a[u] = *(const f32x4*)(prd + base + j);
        b[u] = *(const f32x4*)(tar + base + j);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (idx[u] < plane) {
            const float c = cf * qw[idx[u] / W];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = Rule::grad(c, a[u][e], b[u][e]);
            *(f32x4*)(dprd + base + idx[u]) = o;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------
// planes * slices fits the 32-bit grid index, an element index fits 30 bits
inline bool plane_shape_ok(long planes, int H, int W) {
    return planes > 0 && H > 0 && W > 0 && planes < (1L << 31) / PLANE_MAX_BLOCKS && (long)H * W < (1L << 30);
}

// bytes of a workspace of `floats` fp32 values per (plane, slice); 0 for a non-positive argument (host-only, no HIP call)
inline size_t plane_ws_bytes(int planes, int H, int W, int floats) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)planes * plane_slices(planes) * floats * sizeof(float);
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

// plane_grad_kernel<Rule> over contiguous [BC][H][W] operands, with every check its index map and 16-byte accesses need
template <class Rule>
int plane_grad_launch(const char* who, const float* prd, const float* tar, const float* qw, const float* coef, float* dprd, int BC, int H, int W,
                      void* stream) {
    SWV2_CHECK_ARG(prd && tar && qw && coef && dprd && BC > 0 && H > 0 && W > 0 && W % 4 == 0, "%s: bad argument (W %% 4)", who);
    SWV2_CHECK_ARG((long)H * W < (1L << 30) && BC <= 65535, "%s: plane or B*C too large for the 32-bit index map", who);
    SWV2_CHECK_ARG((((uintptr_t)prd | (uintptr_t)tar | (uintptr_t)dprd) & 15) == 0, "%s: pointer not 16-byte aligned", who);
    hipLaunchKernelGGL(plane_grad_kernel<Rule>, dim3(cdiv((long)H * W, 4096), BC), dim3(256), 0, (hipStream_t)stream, prd, tar, qw, coef, dprd,
                       H, W);
    SWV2_CHECK_LAUNCH(who);
    return SWV2_OK;
}
