// Ensemble scores: CRPS, fair CRPS, spread, ensemble-mean RMSE and the rank histogram of M forecast members x_0 .. x_{M-1} against the
// verifying analysis y, per (sample, channel) plane.  One streaming pass: every thread holds the M values of its grid points in
// registers, so members and truth are read from HBM exactly once (4 (M + 1) B per grid point) and nothing member-sized is written.
//
//   launch 1  ens_sums_kernel<MB, PTS, FULL>    per (plane, slice): four float partial sums and M + 1 integer counts -> workspace
//   launch 2  ens_finalize_kernel               one workgroup per channel: folds the slices, the four scores, the batch means
//
// Per grid point (all terms are formed from DIFFERENCES of inputs; q = w[h]):
//     d_m  = x_m - y                  e1 = sum_m |d_m|                  rank = #{m : x_m < y}   (strict; NaN compares false)
//     a_m  = x_m - x_0                abar = (sum_m a_m) * (1 / M)      v_m = a_m - abar        (x_m - xbar, never from sum x^2)
//     e    = d_0 + abar               (xbar - y)
//     x_(1) <= .. <= x_(M) by a sorting network;  e2 = sum_{i=1}^{M-1} i (M - i) (x_(i+1) - x_(i)) = sum_{m<n} |x_m - x_n|
//   and per plane   S_mse = sum q e^2    S_var = (sum q sum_m v_m^2) / (M - 1)    S_1 = sum q e1    S_2 = sum q e2    hist[rank] += 1.
// The division by M - 1 is done once per plane in ens_finalize_kernel.
//
// Member slots.  The member count M is a runtime value; the register array has MB = M rounded up to a multiple of 8 slots (eight
// compile-time sizes), grouped into the capacities 8 / 16 / 32 / 64 that decide the PTS grid points per thread and iteration:
//     MB 8, 16: PTS 4 (16-byte loads)    MB 24 .. 64: PTS 1 (4-byte loads: a wave reads 256 B per member)
// (MB 24 and 32 were measured with PTS 2 as well: 64 values per thread cost the waves that hide the load latency, M = 32 took 3.09 ms
// instead of 2.39 ms at 73 x 720 x 1440.)  All member loads of an iteration are issued before the first use.  Each size has two kernels:
// FULL (M == MB), where every `m < M` below is a compile-time fact and the gap coefficients are literals, and one for MB - 8 < M < MB,
// where only the last seven slots are guarded by a wave-uniform `m < M`; their unused slots carry +inf, sort to the top and are never
// read: the gap sum stops at i = M - 1 by a branch, not by a zero coefficient, so no 0 * (inf - inf) is formed.
//
// e2 by the gaps of the sorted members at every size: Batcher's odd-even merge sort, pruned to MB inputs, costs 19 / 63 / 191 / 543
// compare-exchanges (two VALU operations each) for 8 / 16 / 32 / 64 slots, i.e. 5 .. 17 operations per loaded value, where the pairwise
// sum costs M - 1 (and M - 1 >= 2 x 19 / 8 only from M = 6 on: below that the two are within a few operations of each other per value
// and one code path is kept); the network needs no runtime index, and min / max are exact, so the only roundings of e2 are the M - 1
// gaps and their fma chain.
//
// Plan and sums: plane_stream.h, with the workgroup index (c * slices + sl) * B + b; a slice without elements stores zeros.  A
// workgroup reads its piece of the truth and of every member once; the neighbours in launch order share the row weights only.  The
// thread's own running sum takes PTS ceil(g / 256) fma, one per grid point, g = groups of PTS elements in the largest slice
// (tests/ensemble_reference.py::chain_length).
//
// Workspace: float part[planes * slices][4], then int cnt[planes * slices][M + 1].  Nothing to zero beforehand: the counts are added
// up in LDS with integer adds (order-independent) and stored by their workgroup.
//
// Per-term roundings, as written below:
//     e1   d_m: 1; M - 1 additions                                         e2   gap: 1; M - 1 fma (the coefficients i (M - i) are exact)
//     v_m  a_m: 1; abar: M - 1 additions + the reciprocal + the product; the subtraction: 1; M fma for sum v^2
//     e    d_0: 1; abar as above; the addition: 1; q e: 1
#include <cmath>

#include "plane_stream.h"

namespace {

constexpr int ENS_MAX_M = 64;

template <int PTS> struct ens_vec;
template <> struct ens_vec<4> { using type = f32x4; };
template <> struct ens_vec<2> { using type = f32x2; };
template <> struct ens_vec<1> { using type = float; };

__device__ __forceinline__ float ens_get(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ float ens_get(const f32x2& v, int e) { return v[e]; }
__device__ __forceinline__ float ens_get(const float& v, int) { return v; }
template <class V> __device__ __forceinline__ V ens_splat(float x);
template <> __device__ __forceinline__ f32x4 ens_splat<f32x4>(float x) { return f32x4{x, x, x, x}; }
template <> __device__ __forceinline__ f32x2 ens_splat<f32x2>(float x) { return f32x2{x, x}; }
template <> __device__ __forceinline__ float ens_splat<float>(float x) { return x; }

// Batcher's odd-even merge sort, ascending, on the first MB of CAP = 2^k register slots (CAP the power of two at or above MB): the
// slots MB .. CAP - 1 stand for +inf, so every compare-exchange that touches one of them is a no-op and is left out -- what remains is
// a sorting network for MB inputs.  Every index is a compile-time constant after unrolling.
template <int CAP, int MB>
__device__ __forceinline__ void ens_sort(float (&x)[MB]) {
#pragma unroll
    for (int p = 1; p < CAP; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < MB; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; ++i)
                    if (i + j + k < MB && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const float lo = fminf(x[i + j], x[i + j + k]), hi = fmaxf(x[i + j], x[i + j + k]);
                        x[i + j] = lo;
                        x[i + j + k] = hi;
                    }
}

struct ens_coef_t { float c[ENS_MAX_M]; };   // c[i] = i (M - i): passed by value, so the kernel reads them as scalars from its argument segment

// MB: the register slots, M rounded up to a multiple of 8.  Slots below LO hold a member whatever M is; only the last seven (six at
// MB = 8, where M starts at 2) are looked at with a wave-uniform `m < M`.
template <int MB, int PTS, bool FULL>
__global__ __launch_bounds__(256) void ens_sums_kernel(const ens_coef_t coef, const float* __restrict__ ens, long ens_ms, long ens_bs,
                                                       const float* __restrict__ tar, long tar_bs, const float* __restrict__ w,
                                                       float* __restrict__ part, int* __restrict__ cnt, int Mrt, int B, int C, int H, int W,
                                                       int slices) {
    using V = typename ens_vec<PTS>::type;
    constexpr int CAP = MB <= 8 ? 8 : MB <= 16 ? 16 : MB <= 32 ? 32 : 64;
    constexpr int LO = FULL ? MB : MB == 8 ? 2 : MB - 7;      // MB - 8 < M <= MB (2 <= M <= 8 at MB = 8)
    const int M = FULL ? MB : Mrt;
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* x0p = ens + b * ens_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    __shared__ int hist[ENS_MAX_M + 1];
    __shared__ float r[4][4];
    if (threadIdx.x <= ENS_MAX_M) hist[threadIdx.x] = 0;
    __syncthreads();
    const float inv_m = 1.0f / (float)M;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    // lo, hi and the slice length are multiples of 4, PTS divides 4: a group of PTS elements never straddles hi or a latitude row
    for (uint32_t i = lo + threadIdx.x * PTS; i < hi; i += 256 * PTS) {
        // one wave-uniform base per member plus the lane's 32-bit byte offset (i < 2^30): the address costs no vector arithmetic
        const uint32_t ib = i * 4;
        V xv[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (m >= LO) xv[m] = ens_splat<V>(INFINITY);
            if (m < LO || m < M) xv[m] = *(const V*)((const char*)(x0p + m * ens_ms) + ib);
        }
        const V yv = *(const V*)((const char*)t + ib);
        const float q = w[i / (uint32_t)W];
#pragma unroll
        for (int e = 0; e < PTS; ++e) {
            float x[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) x[m] = ens_get(xv[m], e);
            const float y = ens_get(yv, e);
            const float d0 = x[0] - y;
            float e1 = fabsf(d0), asum = 0.f;
            int rank = x[0] < y ? 1 : 0;
#pragma unroll
            for (int m = 1; m < MB; ++m)
                if (m < LO || m < M) {
                    e1 += fabsf(x[m] - y);
                    rank += x[m] < y ? 1 : 0;
                    asum += x[m] - x[0];
                }
            const float abar = asum * inv_m;
            float vv = abar * abar;                            // v_0 = a_0 - abar = -abar
#pragma unroll
            for (int m = 1; m < MB; ++m)
                if (m < LO || m < M) {
                    const float v = (x[m] - x[0]) - abar;
                    vv = fmaf(v, v, vv);
                }
            const float em = d0 + abar;
            ens_sort<CAP, MB>(x);
            float e2 = 0.f;
#pragma unroll
            for (int i2 = 1; i2 < MB; ++i2)
                if (i2 < LO || i2 < M) e2 = fmaf(FULL ? (float)(i2 * (MB - i2)) : coef.c[i2], x[i2] - x[i2 - 1], e2);
            s[0] = fmaf(q * em, em, s[0]);
            s[1] = fmaf(q, vv, s[1]);
            s[2] = fmaf(q, e1, s[2]);
            s[3] = fmaf(q, e2, s[3]);
            atomicAdd(&hist[rank], 1);                         // LDS, integer: 0 <= rank <= M
        }
    }
    plane_block_stage(s, r);                                   // after its barrier the wave sums and every count of this workgroup are in LDS
    const size_t slot = (size_t)(b * C + c) * slices + sl;
    if (threadIdx.x == 0) {
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = plane_block_total(r[k]);
        *(f32x4*)(part + slot * 4) = o;
    }
    if ((int)threadIdx.x <= M) cnt[slot * (size_t)(M + 1) + threadIdx.x] = hist[threadIdx.x];
}

// One workgroup per channel: wave v folds the planes b = v, v + 4, ...: the float partials by plane_fold_slices, the counts with
// lane = rank (integers: any order gives the same); lane 0 writes the plane's sums and scores; thread 0 then adds the B values of the
// channel in ascending b for the batch means.
__global__ __launch_bounds__(256) void ens_finalize_kernel(const float* __restrict__ part, const int* __restrict__ cnt, int slices, int M, int B, int C,
                                                           float npix, const float* __restrict__ scale, float* __restrict__ sums,
                                                           int* __restrict__ hist, float* ens_rmse, float* spread, float* crps, float* fair_crps,
                                                           float* __restrict__ means) {
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    const float fm = (float)M;
    for (int b = threadIdx.x >> 6; b < B; b += 4) {
        const size_t pl = (size_t)b * C + c;
        for (int k = lane; k <= M; k += 64) {
            int n = 0;
            for (int sl = 0; sl < slices; ++sl) n += cnt[(pl * slices + sl) * (size_t)(M + 1) + k];
            hist[pl * (M + 1) + k] = n;
        }
        f32x4 a;
        plane_fold_slices<1>((const f32x4*)part, pl, slices, lane, &a);
        if (lane == 0) {
            a[1] = a[1] / (fm - 1.0f);
            *(f32x4*)(sums + pl * 4) = a;
            ens_rmse[pl] = sqrtf(a[0] / npix);
            // S_1 holds every member and the truth: a NaN there poisons all four scores of the plane (the spread too, which the truth
            // does not enter otherwise)
            spread[pl] = a[2] != a[2] ? a[2] : sqrtf(a[1] / npix);
            const float t1 = a[2] / fm;
            crps[pl] = (t1 - a[3] / (fm * fm)) / npix;
            fair_crps[pl] = (t1 - a[3] / (fm * (fm - 1.0f))) / npix;
        }
    }
    __syncthreads();                                       // the plane values above are this workgroup's own global stores
    if (threadIdx.x < 4) {
        const float* v = threadIdx.x == 0 ? ens_rmse : threadIdx.x == 1 ? spread : threadIdx.x == 2 ? crps : fair_crps;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += v[(size_t)b * C + c];
        acc /= (float)B;
        means[threadIdx.x * C + c] = (scale && threadIdx.x < 3) ? acc * scale[c] : acc;
    }
}

template <int MB, int PTS>
void ens_launch(dim3 grid, hipStream_t st, const float* ens, long ms, long bs, const float* tar, long tbs, const float* w, float* part, int* cnt,
                int M, int B, int C, int H, int W, int slices) {
    ens_coef_t coef;
    for (int i = 0; i < ENS_MAX_M; ++i) coef.c[i] = i < M ? (float)(i * (M - i)) : 0.f;
    if (M == MB)
        hipLaunchKernelGGL((ens_sums_kernel<MB, PTS, true>), grid, dim3(256), 0, st, coef, ens, ms, bs, tar, tbs, w, part, cnt, M, B, C, H, W, slices);
    else
        hipLaunchKernelGGL((ens_sums_kernel<MB, PTS, false>), grid, dim3(256), 0, st, coef, ens, ms, bs, tar, tbs, w, part, cnt, M, B, C, H, W, slices);
}

// The workspace, carved here and nowhere else (offsets in 4-byte words): float part[slots][4], then int cnt[slots][M + 1].  swv2_ens_sums,
// swv2_ens_finalize and swv2_ens_ws_bytes all go through it.
struct ens_ws {
    size_t cnt_at, words;
    ens_ws(size_t slots, int M) : cnt_at(slots * 4), words(cnt_at + slots * (M + 1)) {}
    size_t bytes() const { return words * 4; }
    float* part(const void* ws) const { return (float*)ws; }
    int* cnt(const void* ws) const { return (int*)ws + cnt_at; }
};

}  // namespace

extern "C" size_t swv2_ens_ws_bytes(int planes, int H, int W, int M) {
    if (planes <= 0 || H <= 0 || W <= 0 || M < 2 || M > ENS_MAX_M) return 0;
    return ens_ws((size_t)planes * plane_slices(planes), M).bytes();
}

extern "C" int swv2_ens_sums(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* w, int M, int B,
                             int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(ens && tar && w && ws, "ens_sums: null pointer");
    SWV2_CHECK_ARG(M >= 2 && M <= ENS_MAX_M, "ens_sums: members M outside 2 .. 64");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "ens_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "ens_sums: W % 4 != 0");
    SWV2_CHECK_ARG(ens_mstride % 4 == 0, "ens_sums: member stride not a multiple of 4");
    if (!plane_operands_ok("ens_sums", {ens, tar, ws}, {ens_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes, swv2_ens_ws_bytes(B * C, H, W, M),
                           "swv2_ens_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const size_t slots = (size_t)B * C * slices;
    const dim3 grid((unsigned)slots);
    const ens_ws lay(slots, M);
    float* part = lay.part(ws);
    int* cnt = lay.cnt(ws);
    hipStream_t st = (hipStream_t)stream;
#define ENS_CASE(MB, PTS) \
    case MB: ens_launch<MB, PTS>(grid, st, ens, ens_mstride, ens_bstride, tar, tar_bstride, w, part, cnt, M, B, C, H, W, slices); break
    switch ((M + 7) / 8 * 8) {
        ENS_CASE(8, 4);
        ENS_CASE(16, 4);
        ENS_CASE(24, 1);
        ENS_CASE(32, 1);
        ENS_CASE(40, 1);
        ENS_CASE(48, 1);
        ENS_CASE(56, 1);
        ENS_CASE(64, 1);
    }
#undef ENS_CASE
    SWV2_CHECK_LAUNCH("swv2_ens_sums");
    return SWV2_OK;
}

extern "C" int swv2_ens_finalize(const void* ws, size_t ws_bytes, int M, int B, int C, int H, int W, const float* scale, float* sums, int* hist,
                                 float* ens_rmse, float* spread, float* crps, float* fair_crps, float* means, void* stream) {
    SWV2_CHECK_ARG(ws && sums && hist && ens_rmse && spread && crps && fair_crps && means, "ens_finalize: null pointer");
    SWV2_CHECK_ARG(M >= 2 && M <= ENS_MAX_M, "ens_finalize: members M outside 2 .. 64");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "ens_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("ens_finalize", {ws, sums}, {}, 1, 0, ws_bytes, swv2_ens_ws_bytes(B * C, H, W, M), "swv2_ens_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const ens_ws lay((size_t)B * C * slices, M);
    const float* part = lay.part(ws);
    const int* cnt = lay.cnt(ws);
    hipLaunchKernelGGL(ens_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, part, cnt, slices, M, B, C, (float)((long)H * W), scale, sums,
                       hist, ens_rmse, spread, crps, fair_crps, means);
    SWV2_CHECK_LAUNCH("swv2_ens_finalize");
    return SWV2_OK;
}
